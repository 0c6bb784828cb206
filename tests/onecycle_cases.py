"""The stand-in module tree of the one-cycle recipe's golden (tools/gen_onecycle_golden.py -> tests/golden/onecycle.npz) and its loader, shared by
the recorder, tests/test_onecycle_cpu.py and tests/test_gpu_onecycle.py.  The tree holds every case of the reference's group layout
(solver/__init__.py:45-58): a leaf conv, a leaf BatchNorm2d, a module that owns a Parameter AND has a child conv (the shape of DCN: its own parameter
is in no group), a leaf holding one frozen parameter, and parameters of 2 * 4096 + 5 and of 7 elements (a chunk boundary and a ragged tensor for
the one-launch update)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "onecycle.npz")
SETTINGS = dict(BASE_LR=3e-3, MOMS=[0.95, 0.85], DIV_FACTOR=10.0, WEIGHT_DECAY=0.01)
STEPS_KEPT = (1, 4, 8)


class Owner(torch.nn.Module):
    """A module with a parameter of its own AND a child: the shape of DCN (weight / bias + conv_offset_mask)."""

    def __init__(self):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(6, 4, 3, 3))
        self.conv_offset_mask = torch.nn.Conv2d(4, 27, 3)


class Holder(torch.nn.Module):
    def __init__(self, n, frozen=False):
        super().__init__()
        self.value = torch.nn.Parameter(torch.empty(n), requires_grad=not frozen)


class Tree(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.bn = torch.nn.BatchNorm2d(8)
        self.dcn = Owner()
        self.frozen = Holder(5, frozen=True)
        self.long = Holder(2 * 4096 + 5)
        self.short = Holder(7)


def make_tree(seed=11):
    m = Tree()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g))
    return m



def load_golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g["param_groups"] = json.loads(str(g["param_groups"]))
    return g


def golden_tree(g, device="cpu"):
    """The tree at the golden's initial values."""
    m = Tree()
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(torch.from_numpy(g["init/" + n]))
    return m.to(device)


def set_grads(m, g, it):
    for n, p in m.named_parameters():
        if p.requires_grad:
            p.grad = torch.from_numpy(g["grad/%d/%s" % (it, n)]).to(p.device)


def rel(x, y):
    """max |difference| / max |value| (y: the golden's array)."""
    y = torch.as_tensor(y, device=x.device)
    return float((x.detach() - y).abs().max() / y.abs().max().clamp(min=1e-30))
