#!/usr/bin/env python3
"""Golden vectors for the patch terms of the zipnerf training loop (s-nerfpp/zipnerf/train.py:280-293): runs the REFERENCE's
edge_aware_loss_v2 and edge_aware_loss_for_semantic (internal/train_utils.py:297-315, 337-359) exactly as train.py calls them, on
seeded patches, and records inputs, the two term values and their autograd gradients as tests/golden/g32_smooth_zip.npz -- the path C
member of the g32_smooth family of oracle/gen_golden_smooth.py.  Build-container only (needs /root/reference).

train_utils.py imports its sibling modules and torch_scatter at module level; the two functions use none of them, so every module of
that list that does not import here is replaced by an empty stand-in."""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)
from oracle import common as _oracle_common  # noqa: E402  (save_golden: writes the fixture, or compares under --check)
OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference/s-nerfpp/zipnerf"
P, PATCH, C = 5, 6, 19
D_MULT = S_MULT = 0.001                      # smo_lam, s_lam of train.py:281-282


class _Stub(types.ModuleType):               # modules the two loss functions never call
    __path__ = []

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return type(k, (), {})


def load_train_utils():
    names = ["internal." + n for n in ("camera_utils", "configs", "datasets", "image", "math", "models", "ref_utils", "stepfun", "utils")]
    for name in ["internal", "torch_scatter"] + names:
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    for name in names:
        setattr(sys.modules["internal"], name.split(".")[1], sys.modules[name])
    spec = importlib.util.spec_from_file_location("internal.train_utils", os.path.join(REF, "internal", "train_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present")
    train_utils = load_train_utils()
    g = torch.Generator().manual_seed(33)
    shape = [P, PATCH, PATCH]
    rgb = torch.rand(*shape, 3, generator=g)
    depth = (torch.rand(*shape, 1, generator=g) * 39.5 + 0.5).requires_grad_(True)
    sem = torch.softmax(torch.randn(*shape, C, generator=g) * 2.0, -1).requires_grad_(True)
    mask = (torch.rand(*shape, 1, generator=g) < 0.3).float()              # the batch's convention: > 0 = masked out
    # train.py:283-293, with num_patch = P rows of the batch
    mask_patch = torch.where(mask > 0, 0, 1)
    dep_patch = depth.reshape(*shape, -1)
    smoothness_loss = train_utils.edge_aware_loss_v2(rgb, 1 / (dep_patch + 1e-5), mask=mask_patch)
    sem_smooth = train_utils.edge_aware_loss_for_semantic(rgb, sem, mask=mask_patch)
    d_smo = torch.nan_to_num(D_MULT * smoothness_loss)
    s_smo = torch.nan_to_num(S_MULT * sem_smooth)
    g_depth, g_sem = torch.autograd.grad(d_smo + s_smo, [depth, sem])
    valid = mask_patch[..., 0] > 0
    nx, ny = int((valid[:, :, :-1] & valid[:, :, 1:]).sum()), int((valid[:, :-1] & valid[:, 1:]).sum())
    assert nx > 0 and ny > 0, (nx, ny)
    _oracle_common.save_golden(os.path.join(OUT, "g32_smooth_zip.npz"), rgb=rgb.numpy(), depth=depth.detach().numpy()[..., 0], sem=sem.detach().numpy(),
                               mask=mask.numpy()[..., 0], d_smo=d_smo.detach().numpy(), s_smo=s_smo.detach().numpy(), g_depth=g_depth.numpy()[..., 0],
                               g_sem=g_sem.numpy(), n_edges=np.asarray([nx, ny], dtype=np.int64), mults=np.asarray([D_MULT, S_MULT], dtype=np.float32))
    print(f"wrote g32_smooth_zip.npz: d_smo {d_smo.item():.6e} s_smo {s_smo.item():.6e} Nx {nx} Ny {ny}")


if __name__ == "__main__":
    main()
