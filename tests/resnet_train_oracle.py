"""TEST INFRASTRUCTURE ONLY -- CPU restatement (PyTorch fp32, functional over a state_dict) of the reference's image encoder
with its BatchNorms in TRAINING mode, as the reference's loop runs it (``encoder.train()`` and the call under ``no_grad``,
My_cross_attention.py:791-805): every nn.BatchNorm2d normalises with the batch's statistics and moves its running
statistics in place (F.batch_norm(training=True)) and its num_batches_tracked counter.  Pinned against the reference's own
resnet/ classes by tests/golden/make_golden_resnet_train.py (fixtures tests/golden/resnet_train_*.npz)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
State = Dict[str, Tensor]


def bn_train(x: Tensor, S: State, prefix: str, momentum: Optional[float] = 0.1, eps: float = 1e-5) -> Tensor:
    """nn.BatchNorm2d.forward in training mode with track_running_stats=True (momentum None: cumulative average)."""
    S[prefix + ".num_batches_tracked"] += 1
    m = 1.0 / float(S[prefix + ".num_batches_tracked"]) if momentum is None else momentum
    return F.batch_norm(x, S[prefix + ".running_mean"], S[prefix + ".running_var"], S[prefix + ".weight"],
                        S[prefix + ".bias"], True, m, eps)


def bn_eval(x: Tensor, S: State, prefix: str, eps: float = 1e-5) -> Tensor:
    return F.batch_norm(x, S[prefix + ".running_mean"], S[prefix + ".running_var"], S[prefix + ".weight"],
                        S[prefix + ".bias"], False, 0.0, eps)


def features(S: State, layers: Sequence[int], x: Tensor, train: bool, momentum: Optional[float] = 0.1,
             eps: float = 1e-5) -> Tensor:
    """ResNet stem + layer1..4 (resnet/resnet.py:139-147, Bottleneck.forward :74-93); train=True updates S in place."""
    bn = (lambda t, p: bn_train(t, S, p, momentum, eps)) if train else (lambda t, p: bn_eval(t, S, p, eps))
    x = F.max_pool2d(F.relu(bn(F.conv2d(x, S["conv1.weight"], stride=2, padding=3), "bn1")), 3, 2, 1)
    for li, n in enumerate(layers):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            p = "layer%d.%d" % (li + 1, bi)
            out = F.relu(bn(F.conv2d(x, S[p + ".conv1.weight"]), p + ".bn1"))
            out = F.relu(bn(F.conv2d(out, S[p + ".conv2.weight"], stride=s, padding=1), p + ".bn2"))
            out = bn(F.conv2d(out, S[p + ".conv3.weight"]), p + ".bn3")
            res = x
            if p + ".downsample.0.weight" in S:
                res = bn(F.conv2d(x, S[p + ".downsample.0.weight"], stride=s), p + ".downsample.1")
            x = F.relu(out + res)
    return x


def my_resnet(S: State, layers: Sequence[int], x: Tensor, train: bool, momentum: Optional[float] = 0.1,
              eps: float = 1e-5) -> Tuple[Tensor, Tensor]:
    """myResnet.forward (resnet/resnet_utils.py:13-53) at 224x224: (fc = spatial mean, att = the 7x7 map)."""
    f = features(S, layers, x, train, momentum, eps)
    return f.mean(3).mean(2), F.adaptive_avg_pool2d(f, [7, 7])


def bn_prefixes(S: State):
    return sorted(k[:-len(".running_mean")] for k in S if k.endswith(".running_mean"))
