"""batching.DrawCounter, the place in the batch stream that the five device batchers share: its checks, its checkpoint and its
snapshot / restore on a stub without a device; on the device, that a restored batcher of every family draws the same batch again and
that a rank's batch is its rows of the single-GPU batch."""
import types

import numpy as np
import pytest
import torch

from snerf_amd import batching

gpu = pytest.mark.gpu


class _Stub(batching.DrawCounter):
    """a batcher whose draw does on the host what the kernels do to the counter's step word"""

    def buffers(self):
        return {"step": torch.empty(1, dtype=torch.int64)}

    def next_into(self, buf):
        buf["step"].copy_(self.counter[:1])
        self.counter += torch.tensor([1, 0])
        return self._drawn(buf)


def test_bad_seed_rank_and_world_are_refused():
    for kw in (dict(seed=-1), dict(seed=1 << 63), dict(rank=-1), dict(rank=1), dict(rank=2, world=2), dict(world=0), dict(rank=0, world=-1)):
        with pytest.raises(ValueError):
            _Stub(16, device="cpu", **kw)
    b = _Stub(16, seed=(1 << 63) - 1, rank=1, world=2, device="cpu")
    assert (b.seed, b.rank, b.world, b.device) == ((1 << 63) - 1, 1, 2, torch.device("cpu"))
    assert b.counter.dtype == torch.int64 and b.counter.tolist() == [0, 0] and b.step == 0


@pytest.mark.parametrize("n, world", [(16, 1), (16, 2), (17, 3), (5, 4), (3, 8)])
def test_the_slice_is_shard_bounds(n, world):
    edges = []
    for rank in range(world):
        b = _Stub(n, rank=rank, world=world, device="cpu")
        assert (b.i0, b.i1) == batching.shard_bounds(n, rank, world) and b.n_rows == b.i1 - b.i0
        edges.append((b.i0, b.i1))
    assert edges[0][0] == 0 and edges[-1][1] == n and all(a[1] == c[0] for a, c in zip(edges, edges[1:]))


def test_state_dict_round_trip():
    a = _Stub(16, seed=7, device="cpu")
    for _ in range(3):
        a.next()
    a.counter[1] = 5                                     # (a ticket left over must not survive the checkpoint)
    sd = a.state_dict()
    assert sd == {"seed": 7, "step": 3}
    b = _Stub(16, seed=1, device="cpu")
    b.load_state_dict(sd)
    assert (b.seed, b.step) == (7, 3) and b.counter.tolist() == [3, 0]
    assert int(b.next()["step"]) == 3 and b.step == 4 and b.counter.tolist() == [4, 0]


def test_snapshot_and_restore_rewind_counter_and_mirror():
    b = _Stub(16, device="cpu")
    b.next()
    snap = b.snapshot()
    assert int(b.next()["step"]) == 1 and int(b.next()["step"]) == 2
    b.advance_host(3)
    assert b.step == 6 and b.counter.tolist() == [3, 0]
    b.restore(snap)
    assert b.step == 1 and b.counter.tolist() == [1, 0]
    assert int(b.next()["step"]) == 1                    # the snapshot is a copy: the draws after it left it alone
    b.restore(snap)
    assert b.step == 1 and b.counter.tolist() == [1, 0]


def test_trainer_re_exports_the_shard_functions():
    from snerf_amd import trainer
    assert trainer.shard_bounds is batching.shard_bounds
    assert trainer.shard_rays is batching.shard_rays and trainer.shard_batch is batching.shard_batch


# ---- GPU: the five batchers ----------------------------------------------------------------------------------------------------------
def _mip(patches):
    def make(rank, world):
        from snerf_amd import sample_utils as su
        rng = np.random.default_rng(0)
        N, H, W = 2, 8, 10
        images, depths = rng.random((N, H, W, 3), dtype=np.float32), (rng.random((N, H, W)) * 60 + 2).astype(np.float32)
        poses = np.tile(np.eye(4, dtype=np.float32)[:3], (N, 1, 1))
        poses[:, :, 3] = rng.normal(size=(N, 3))
        K = np.tile(np.array([[30, 0, W / 2], [0, 30, H / 2], [0, 0, 1]], np.float32), (N, 1, 1))
        args = types.SimpleNamespace(no_ndc=True, smooth_loss=patches, near_far=False, N_rgb=16)
        kw = dict(batch_n=16, seed=3, rank=rank, world=world, device="cuda")
        if patches:
            return su.PatchRayBatcher(args, images, depths, poses, K, [0, 1], 2.0, 80.0, patch_sz=2, n_patch=2, **kw)
        return su.ImageRayBatcher(args, images, depths, poses, K, [0, 1], 2.0, 80.0, **kw)

    def rows(b, g):
        """rows of the single-GPU batch (of batcher g) that b draws"""
        r = list(range(b.i0, b.i1))
        if patches:
            r += list(range(g.n_rgb_rows + b.k0 * b.patch_sz ** 2, g.n_rgb_rows + b.k1 * b.patch_sz ** 2))
        return r
    return make, rows


def _classic():
    def make(rank, world):
        from snerf_amd import classic
        rng = np.random.default_rng(0)
        images = rng.integers(0, 256, size=(2, 4, 4, 3), dtype=np.uint8)
        poses = np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1))
        poses[:, :, 3] = rng.normal(size=(2, 3))
        return classic.RayBatcher(images, poses, 5.0, [0, 1], 8, near=2.0, far=6.0, ndc=False, use_viewdirs=True, seed=3, rank=rank, world=world,
                                  device="cuda")
    return make, lambda b, g: list(range(b.i0, b.i1))


def _zip(patches):
    def make(rank, world):
        from snerf_amd import zipnerf
        rng = np.random.default_rng(0)
        N, H, W = 2, 8, 8
        images = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
        K = np.tile(np.array([[40, 0, W / 2], [0, 40, H / 2], [0, 0, 1]], np.float64), (N, 1, 1))
        c2w = np.tile(np.eye(4, dtype=np.float32)[:3], (N, 1, 1))
        c2w[:, :, 3] = rng.normal(size=(N, 3)) * 0.05
        kw = dict(batch_size=64, seed=3, rank=rank, world=world, device="cuda")
        if patches:
            return zipnerf.PatchRayBatcher(images, np.linalg.inv(K).astype(np.float32), c2w, 0.02, 100.0, 2, **kw)
        return zipnerf.RayBatcher(images, np.linalg.inv(K).astype(np.float32), c2w, 0.02, 100.0, **kw)

    def rows(b, g):
        r = list(range(b.i0, b.i1))
        if patches:
            r = list(range(b.k0 * b.patch_size ** 2, b.k1 * b.patch_size ** 2)) + r
        return r
    return make, rows


def _tensors(buf):
    """{name: (tensor, axis of the batch rows or None)} of one drawn batch"""
    out = {}
    for k, v in buf.items():
        if v is not None:
            out[k] = (v, None if k == "img" else 1 if k == "extras" else 0)
    return out


@gpu
@pytest.mark.parametrize("family", ["mip-pixels", "mip-patches", "classic", "zip-pixels", "zip-patches"])
def test_restored_batcher_redraws_the_batch_and_a_rank_draws_its_rows(family):
    make, rows = {"mip-pixels": lambda: _mip(False), "mip-patches": lambda: _mip(True), "classic": _classic, "zip-pixels": lambda: _zip(False),
                  "zip-patches": lambda: _zip(True)}[family]()
    g = make(0, 1)
    g.next()                                             # (not from step 0: the snapshot holds a place, not zeros)
    snap = g.snapshot()
    buf = g.buffers()
    g.next_into(buf)
    first = {k: (v.clone(), ax) for k, (v, ax) in _tensors(buf).items()}
    assert g.step == 2 and g.counter.tolist() == [2, 0]
    assert first and all(v.shape[ax] == g.n_rows for v, ax in first.values() if ax is not None)
    g.restore(snap)
    assert g.step == 1 and g.counter.tolist() == [1, 0]
    again = g.buffers()
    g.next_into(again)
    assert g.step == 2 and g.counter.tolist() == [2, 0]
    for k, (v, _) in _tensors(again).items():
        assert torch.equal(v.view(torch.uint8), first[k][0].view(torch.uint8)), k

    b = make(1, 2)
    assert (b.rank, b.world) == (1, 2) and (b.i0, b.i1) != (g.i0, g.i1)
    b.next()
    mine = b.buffers()
    b.next_into(mine)
    idx = torch.as_tensor(rows(b, g), device="cuda")
    assert idx.numel() == b.n_rows and 0 < b.n_rows < g.n_rows
    for k, (v, ax) in _tensors(mine).items():
        want = first[k][0] if ax is None else first[k][0].index_select(ax, idx)
        assert torch.equal(v.view(torch.uint8), want.view(torch.uint8)), k
