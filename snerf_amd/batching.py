"""What the device ray batchers share, and the split of a batch over the ranks.  Imports nothing of the package: the trainers and the
modules that hold the batchers (sample_utils, classic, zipnerf) all build on it."""
import torch


def shard_bounds(n: int, rank: int, world: int):
    """[start, end) of rank's contiguous share of n rays; the first n % world ranks take one extra ray, nothing is dropped."""
    per, rem = divmod(n, world)
    start = rank * per + min(rank, rem)
    return start, start + per + (1 if rank < rem else 0)


def shard_rays(rays, rank: int, world: int):
    """Contiguous split of a ray batch (namedtuple of [N,.] tensors) across ranks; see shard_bounds."""
    a, b = shard_bounds(rays[0].shape[0], rank, world)
    return type(rays)(*[r[a:b] for r in rays])


def shard_batch(rays, rank: int, world: int, *per_ray):
    """shard_rays for the rays AND every per-ray target (target_rgb, target_depth, conf, ...; None passes through) with the same
    bounds, so that a caller cannot slice them inconsistently.  -> (rays_shard, *target_shards)"""
    a, b = shard_bounds(rays[0].shape[0], rank, world)
    for t in per_ray:
        if t is not None and t.shape[0] != rays[0].shape[0]:
            raise ValueError("per-ray tensor does not match the ray batch")
    return (type(rays)(*[r[a:b] for r in rays]),) + tuple(None if t is None else t[a:b] for t in per_ray)


class DrawCounter:
    """The place a device batcher keeps in its endless stream of batches: `counter`, the int64 {step, workgroup ticket} pair in device
    memory that every draw launch reads and advances, its host mirror `step`, the `seed` of the counter-based generator, and rows
    [i0, i1) = shard_bounds(n, rank, world) of the one global batch of n rows that this rank draws.  A batcher supplies `buffers()`
    (fresh output tensors of one batch) and `next_into(buf)`, which launches the draw on `counter` and returns `self._drawn(...)`."""

    def __init__(self, n, seed=0, rank=0, world=1, device=None):
        seed, rank, world = int(seed), int(rank), int(world)
        if not 0 <= seed < (1 << 63):
            raise ValueError("seed must be in [0, 2^63)")
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank in [0, world)")
        self.seed, self.rank, self.world = seed, rank, world
        self.device = torch.device(device if device is not None else "cuda")
        self.i0, self.i1 = shard_bounds(int(n), rank, world)
        self.counter = torch.zeros(2, dtype=torch.int64, device=self.device)   # {step, workgroup ticket}: advanced by the launch
        self._step = 0

    @property
    def step(self):
        """the step of the next draw (host mirror of the device counter; `advance_host` after graph replays of `next_into`)"""
        return self._step

    @property
    def n_rows(self):
        """rows of this rank's batch"""
        return self.i1 - self.i0

    def state_dict(self):
        return {"seed": self.seed, "step": self._step}

    def load_state_dict(self, sd):
        self.seed, self._step = int(sd["seed"]), int(sd["step"])
        self.counter.copy_(torch.tensor([self._step, 0], dtype=torch.int64))

    def advance_host(self, k=1):
        """tell the host mirror that k draws ran inside graph replays (k = -1: a draw was recorded into a graph, not run)"""
        self._step += int(k)

    def _drawn(self, out):
        """a draw was launched on `counter`: the host mirror follows -> out"""
        self._step += 1
        return out

    def snapshot(self):
        """-> the batcher's place, for `restore` (a warm-up that must use up no draws)"""
        return self.counter.clone(), self._step

    def restore(self, snap):
        """back to the place of `snapshot()`: the device counter (a copy on the current stream) and the host mirror"""
        self.counter.copy_(snap[0])
        self._step = snap[1]

    def next(self):
        """the batch of the next step in new tensors (they stay valid); what `next_into` returns"""
        return self.next_into(self.buffers())
