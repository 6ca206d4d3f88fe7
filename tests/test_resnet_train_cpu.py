"""CPU: the train-mode BatchNorm restatement (tests/resnet_train_oracle.py) against the fixtures produced by the reference's
own resnet/ classes in training mode (tests/golden/make_golden_resnet_train.py), and the opt-in interface of the encoder."""
import numpy as np
import pytest
import torch

import resnet_train_oracle as O
from golden_util import GOLDEN_DIR
from icka_amd import synth


def _state(layers):
    from icka_amd.resnet import Bottleneck, ResNet
    net = ResNet(Bottleneck, list(layers))
    synth.fill_resnet_(net)
    return {k: v.clone() for k, v in net.state_dict().items()}


def _close(a, b, tol=1e-5):
    b = np.asarray(b)
    return np.abs(np.asarray(a) - b).max() <= tol * max(np.abs(b).max(), 1e-30)


def test_train_oracle_matches_reference_fixture():
    z = np.load(GOLDEN_DIR + "/resnet_train_tiny_1111_b2.npz")
    layers, B, seeds = [int(v) for v in z["layers"]], int(z["batch"]), [int(v) for v in z["seeds"]]
    S = _state(layers)
    with torch.no_grad():
        for i in range(2):
            x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seeds[i]))
            fc, att = O.my_resnet(S, layers, x, train=True)
            assert _close(fc.numpy(), z["fc%d" % i]) and _close(att[:, ::16].numpy(), z["att%d_sample" % i])
        for p in O.bn_prefixes(S):
            assert _close(S[p + ".running_mean"].numpy(), z[p + ".running_mean"]), p
            assert _close(S[p + ".running_var"].numpy(), z[p + ".running_var"]), p
            assert int(S[p + ".num_batches_tracked"]) == int(z["num_batches_tracked"])
        x = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seeds[2]))
        fc, _ = O.my_resnet(S, layers, x, train=False)
        assert _close(fc.numpy(), z["fc_eval"])


def test_train_batchnorm_is_opt_in():
    from icka_amd.resnet import resnet50, resnet101, resnet152
    assert resnet50().train_batchnorm is False
    assert resnet101(train_batchnorm=True).train_batchnorm is True
    net = resnet152(train_batchnorm=True)
    assert net.train_batchnorm is True and net.implicit_conv is True
    # same state_dict as the default network (checkpoints load either way)
    assert net.state_dict().keys() == resnet152().state_dict().keys()
