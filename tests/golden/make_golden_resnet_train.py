#!/usr/bin/env python3
"""Generates tests/golden/resnet_train_*.npz from the REFERENCE's own image encoder (resnet/resnet.py + resnet/resnet_utils.py,
imported from /root/reference; dev container only) with its BatchNorms in training mode, as the reference's loop runs it
(``encoder.train()``, the call under ``no_grad``): two train-mode calls on two seeded batches, then one eval-mode call, on
by-key seeded weights (icka_amd.synth.fill_resnet_).  Asserts that tests/resnet_train_oracle.py reproduces it.  The fixtures
hold the inputs' seeds and expected outputs / running statistics only.
usage: python tests/golden/make_golden_resnet_train.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

import resnet_train_oracle as O  # noqa: E402
from icka_amd import synth  # noqa: E402
from resnet import resnet as R  # noqa: E402  (reference)
from resnet.resnet_utils import myResnet  # noqa: E402  (reference)


def images(B, seed):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


def case(name, layers, B, seeds, stride):
    """stride: channel subsampling of the stored running statistics (1 = every channel)."""
    net = R.ResNet(R.Bottleneck, layers)
    synth.fill_resnet_(net)
    S = {k: v.clone() for k, v in net.state_dict().items()}
    enc = myResnet(net, False, torch.device("cpu"))
    out = {"layers": np.array(layers), "batch": B, "seeds": np.array(seeds), "stats_stride": stride}
    with torch.no_grad():
        for i, seed in enumerate(seeds[:2]):
            net.train()
            enc.train()
            _, fc, att = enc(images(B, seed))
            ofc, oatt = O.my_resnet(S, layers, images(B, seed), train=True)
            assert (ofc - fc).abs().max().item() <= 1e-5 * fc.abs().max().item(), "oracle != reference (fc %d)" % i
            assert (oatt - att).abs().max().item() <= 1e-5 * att.abs().max().item(), "oracle != reference (att %d)" % i
            out["fc%d" % i] = fc.numpy()
            out["att%d_sample" % i] = att[:, ::16].numpy()
        net.eval()
        enc.eval()
        _, fc, att = enc(images(B, seeds[2]))
        ofc, _ = O.my_resnet(S, layers, images(B, seeds[2]), train=False)
        assert (ofc - fc).abs().max().item() <= 1e-5 * fc.abs().max().item(), "oracle != reference (eval fc)"
        out["fc_eval"] = fc.numpy()
    sd = net.state_dict()
    for p in O.bn_prefixes(S):
        for leaf in ("running_mean", "running_var"):
            ref = sd[p + "." + leaf]
            assert (S[p + "." + leaf] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), p + "." + leaf
            out[p + "." + leaf] = ref[::stride].numpy()
        assert int(sd[p + ".num_batches_tracked"]) == int(S[p + ".num_batches_tracked"]) == 2
    out["num_batches_tracked"] = 2
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", name + ".npz"), **out)
    print(name, "fc0 max", float(np.abs(out["fc0"]).max()), "fc_eval max", float(np.abs(out["fc_eval"]).max()))


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    case("resnet_train_tiny_1111_b2", [1, 1, 1, 1], 2, [21, 22, 23], 1)
    case("resnet_train_152_b2", [3, 8, 36, 3], 2, [31, 32, 33], 16)
