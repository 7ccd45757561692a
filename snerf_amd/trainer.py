"""Training step for the mip path without the autograd round trip: forward, per-ray loss tail, backward,
gradient exchange and fused Adam on the flat arenas.

Reference counterpart: the hot loop of s-nerf/train.py:110-221 (model forward :112-115, RGB MSE
loss_factory.py:5-11, disparity-L1 depth loss with per-ray confidence loss_factory.py:26-37 /
confidence.py:209-224, ProposalLoss loss_factory.py:59-74, loss.backward() :213, optimizer.step() :217-221).
The per-ray loss tail is one kernel that returns the loss terms and
dL/d(rgb, distance, coarse weights) -- no [N]-sized torch expressions, no device->host sync in the step.

Multi-GPU: one process per GPU, every rank renders its own shard of the ray batch; the only exchange is the
RCCL all-reduce of the flat fp32 gradient arena (35.9 MB for the shipped model), issued network by network as
the backward pass completes each block so that it overlaps with the rest of the backward, before the Adam
kernel, which folds the 1/world_size mean into its pass.
"""
import torch
import torch.distributed as dist

from . import ops
from .batching import shard_batch, shard_bounds, shard_rays      # (re-exported: trainer.shard_bounds and its siblings)


class _GradExchange:
    """Gradient all-reduce overlapped with the backward pass: the arena is laid out network by network and layer by layer, and as soon
    as a block's gradients are final -- the NeRF MLP's heads, then each 4 MB trunk layer as the backward reaches it, then the proposal
    network -- it is all-reduced asynchronously (RCCL runs it on its own stream) while the remaining backward kernels keep the compute
    stream busy: only the last trunk layer's bucket (~0.4 MB) is left exposed in front of Adam.  `finish()` reduces whatever was not
    announced and waits for everything."""

    def __init__(self, arena, world, group, single_rank=False):
        """`single_rank`: run the collectives even in a process group of one rank (diagnostics: exercises the RCCL path on a 1-GPU box)"""
        self.arena, self.world, self.group = arena, world, group
        self.active = world > 1 or single_rank
        self.works, self.done = [], []

    def __call__(self, prefix):
        """`prefix`: a parameter-name prefix or a list of them; neighbouring spans go out as ONE collective, and what an earlier call
        already covered is not sent twice (the backward announces the NeRF MLP layer by layer and then once more as a whole)."""
        if not self.active:
            return
        spans = sorted(self.arena.span(p) for p in ([prefix] if isinstance(prefix, str) else prefix))
        merged = []
        for a, b in spans:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        for a, b in merged:
            # [a, b) minus the union of what is already on the wire, in one sweep over the sent spans in ascending order
            pos = a
            for c, d in sorted(self.done):
                if d <= pos:
                    continue
                if c >= b:
                    break
                if c > pos:
                    self._send(pos, c)
                pos = max(pos, d)
            if pos < b:
                self._send(pos, b)

    def _send(self, x, y):
        self.done.append((x, y))
        self.works.append(dist.all_reduce(self.arena.grad[x:y], op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        if not self.active:
            return
        pos = 0
        for a, b in sorted(self.done) + [(self.arena.numel, self.arena.numel)]:
            if a > pos:
                self.works.append(dist.all_reduce(self.arena.grad[pos:a], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            pos = max(pos, b)
        for w in self.works:
            w.wait()
        self.works, self.done = [], []


class _AdamState:
    """A flat fp32 buffer trained by one fused Adam launch (ops.adam_step): the moments `m` / `v`, the step count `t`, `lr` / `betas` /
    `eps` (plain attributes, read at step time), the device step / lr words of a captured step, and the checkpoint of all that in
    torch.optim.Adam's `state_dict()` layout -- what the reference stores next to the weights (s-nerf/train.py:264-273 'optimzer',
    resumed at utils/model_utils.py:44-63; zipnerf/train.py:432-440 'optimizer', internal/checkpoints.py:52-54): a checkpoint written by
    the reference's training loop resumes here and the other way round
    (`torch.optim.Adam(model.parameters()).load_state_dict(trainer.state_dict())`).
    The class that trains a buffer supplies `_buffers()` -> (parameters, gradients), `_layout()` -> [(name, offset, count, shape)] of the
    parameters in the buffer, and `what`, the buffer's name in messages.  `named`: the checkpoint also names the parameters
    (`param_names`) and is refused for a buffer with other names; without it the checkpoint is torch's plain layout."""
    step_dev = lr_dev = _graph = None               # (step_dev / lr_dev: int32 [1] / fp32 [1] on the device once a captured step holds the Adam)
    named = False

    def _moments(self):
        return self.m, self.v

    def adam(self, grad_scale, nonfinite, lo=None, hi=None, grad=None, **hygiene):
        """the fused Adam launch over the whole buffer, or over its slice [lo, hi) with `grad` (a reduced shard) in place of the buffer's
        own gradient slice; zeroes the gradients it read.  `hygiene`: ops.adam_step's grad_max_val / clip_coef / dropped"""
        flat, g = self._buffers()
        m, v = self.m, self.v
        if lo is not None:
            flat, g, m, v = flat[lo:hi], g[lo:hi], m[lo:hi], v[lo:hi]
        ops.adam_step(flat, g if grad is None else grad, m, v, self.lr, self.betas[0], self.betas[1], self.eps, self.t, grad_scale=grad_scale,
                      zero_grad=True, nonfinite=nonfinite, step_dev=self.step_dev, lr_dev=self.lr_dev, **hygiene)

    def arm(self):
        """step count and learning rate move into device memory, where a captured Adam launch reads them"""
        self.step_dev = torch.tensor([self.t], dtype=torch.int32, device=self.m.device)
        self.lr_dev = torch.tensor([self.lr], dtype=torch.float32, device=self.m.device)

    def snapshot(self):
        return self._buffers()[0].clone(), self.m.clone(), self.v.clone(), self.t

    def restore(self, snap):
        flat, grad = self._buffers()
        with torch.no_grad():
            flat.copy_(snap[0]); self.m.copy_(snap[1]); self.v.copy_(snap[2])
            self.t = snap[3]
            grad.zero_()
            if self.step_dev is not None:
                self.step_dev.fill_(self.t)

    def state_dict(self):
        m, v = self._moments()
        layout = self._layout()
        state = {i: {"step": torch.tensor(float(self.t)), "exp_avg": m[lo:lo + cnt].view(shape).clone(), "exp_avg_sq": v[lo:lo + cnt].view(shape).clone()}
                 for i, (_, lo, cnt, shape) in enumerate(layout)}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(layout)))}
        sd = {"state": state, "param_groups": [group]}
        if self.named:
            sd["param_names"] = [n for n, *_ in layout]
        return sd

    def load_state_dict(self, sd):
        """every check comes before the first write: a refused state leaves the moments, t, lr / betas / eps and the device step word alone"""
        layout = self._layout()
        if self.named and "param_names" in sd and list(sd["param_names"]) != [n for n, *_ in layout]:
            raise ValueError("optimizer state was saved for other parameter names")
        groups = sd["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if len(order) != len(layout):
            raise ValueError(f"{self.what} optimizer state for {len(order)} parameters, {len(layout)} expected ({', '.join(n for n, *_ in layout)})")
        hyper = lambda g: (float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]))
        lr, betas, eps = hyper(groups[0])
        if any(hyper(g) != (lr, betas, eps) for g in groups[1:]):   # one launch, one set of hyper-parameters
            raise ValueError(f"the fused Adam launch covers the {self.what} parameters with one lr / betas / eps: the saved param_groups differ")
        if any(float(g.get("weight_decay", 0) or 0) != 0 or g.get("amsgrad", False) for g in groups):
            raise ValueError("the fused Adam launch has no weight decay / amsgrad")
        if (self.step_dev is not None or self._graph is not None) and (betas, eps) != (tuple(float(b) for b in self.betas), float(self.eps)):
            # betas / eps are host kernel arguments baked into the captured hipGraph (lr and the step count live on the device)
            raise ValueError("load_state_dict after capture(): the checkpoint's betas / eps differ from the captured step's -- load before capturing")
        saved, steps = [], set()
        for pos, (name, _, _, shape) in zip(order, layout):
            st = sd["state"].get(pos, sd["state"].get(str(pos)))    # (None: a parameter the saved optimizer never stepped)
            if st is not None:
                for key in ("exp_avg", "exp_avg_sq"):
                    if tuple(st[key].shape) != tuple(shape):
                        raise ValueError(f"{self.what} optimizer state of {name}: {key} has shape {tuple(st[key].shape)}, the parameter has {tuple(shape)}")
                steps.add(int(float(st["step"])))
            saved.append(st)
        if len(steps) > 1:
            raise ValueError(f"one Adam launch covers the {self.what} parameters: the saved parameters disagree on the step count ({sorted(steps)})")
        with torch.no_grad():
            for st, (_, lo, cnt, _) in zip(saved, layout):
                for buf, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq")):
                    if st is None:
                        buf[lo:lo + cnt].zero_()
                    else:
                        buf[lo:lo + cnt].copy_(st[key].reshape(-1).to(buf.device, torch.float32))
        self.t = steps.pop() if steps else 0
        self.lr, self.betas, self.eps = lr, betas, eps
        if self.step_dev is not None:
            self.step_dev.fill_(self.t)


class _CapturedStep:
    """hipGraph capture and replay of a trainer's whole step: what MipTrainer and ClassicTrainer share.  The trainer's `capture()` does
    its refusals and wires the batch tensors, then hands `_capture` the two bodies; it supplies `_trained()` (the _AdamStates of the
    step's Adam launches), `_counted()` where other objects hold the step counts, `_bump_restored()` and `_after_graph()`."""
    _batcher = None

    def _counted(self):
        """the objects whose `t` one step advances by one"""
        return self._trained()

    def _capture(self, warmup, batcher, buf, step, forward_backward):
        """`step()` / `forward_backward()` -> (loss, outs) on the capture batch; `batcher.next_into(buf)` runs ahead of either.  The
        `warmup` steps are real steps on a side stream, with the trained states and the batcher's place snapshotted before and restored
        after them; then the graph records `step` (world 1, step counts and learning rates armed in device memory) or
        `forward_backward` (world > 1: `replay()` follows the graph with `_after_graph()`).  -> the graph's loss tensor"""
        dev = self.m.device
        trained = self._trained()
        snaps = [x.snapshot() for x in trained]
        if self.world == 1:
            for x in trained:
                x.arm()
        self._batcher = batcher
        b_snap = None if batcher is None else batcher.snapshot()

        def draw():
            if batcher is not None:
                batcher.next_into(buf)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                    # warm-up on a side stream
            for _ in range(warmup):
                draw()
                step()
        torch.cuda.current_stream(dev).wait_stream(side)
        for x, snap in zip(trained, snaps):
            x.restore(snap)
        if batcher is not None:                          # capturing uses up no draws
            batcher.restore(b_snap)
        self._bump_restored()                            # (the restored parameters are new values to the packed operands)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            draw()
            self._graph_loss, self._graph_outs = step() if self.world == 1 else forward_backward()
        if batcher is not None:
            batcher.advance_host(-1)                     # capturing records the draw and the step, it does not run them
        if self.world == 1:
            for x in self._counted():
                x.t -= 1
        return self._graph_loss

    def replay(self):
        """One captured step.  -> (loss, outs): the same device tensors every time, overwritten by each replay."""
        if self._batcher is not None:
            self._batcher.advance_host(1)                # the graph's first node drew the batch and advanced the device counter
        if self.world == 1:
            for x in self._trained():
                x.lr_dev.fill_(x.lr)                     # the graph reads the learning rates from the device
            self._graph.replay()
            for x in self._counted():
                x.t += 1
        else:
            self._graph.replay()                         # forward + loss tail + backward of this rank's shard
            self._after_graph()                          # the gradient exchange and the Adam launches
        return self._graph_loss, self._graph_outs


class _ArenaAdam(_AdamState):
    """_AdamState over a model's flat arena, in the order of `model.parameters()`: what MipTrainer and ZipTrainer share.  The checkpoint
    also names the parameters (`param_names`) and is refused for a model with other names."""
    what, named = "model", True
    side = ()                                       # (the side tables trained beside the model: MipTrainer's)
    _step_dev, _lr_dev = property(lambda self: self.step_dev), property(lambda self: self.lr_dev)

    def _arena_buffers(self, model, lr, betas, eps, nonfinite, grad_max_val, grad_max_norm, process_group):
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.nonfinite, self.grad_max_val, self.grad_max_norm = nonfinite, float(grad_max_val), float(grad_max_norm)
        self.m, self.v, self.t = torch.zeros_like(model.arena.flat), torch.zeros_like(model.arena.flat), 0
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        model.arena.grad.zero_()

    def _buffers(self):
        return self.model.arena.flat, self.model.arena.grad

    def broadcast_parameters(self, src=0):
        if self.world > 1:
            dist.broadcast(self.model.arena.flat, src=src, group=self.pg)
            self.model.arena.bump()
            for table in self.side:
                for p in table.broadcast_tensors():
                    dist.broadcast(p, src=src, group=self.pg)

    def _layout(self):
        a = self.model.arena
        return [(n, *a._offs[n], a.shapes[n]) for n, _ in self.model.named_parameters()]

    def _arena_adam(self, grad_scale, **hygiene):
        """one fused Adam launch over the flat arena; folds `grad_scale` (the data-parallel mean, the loss scale), the gradient hygiene and
        zero_grad"""
        a = self.model.arena
        coef = ops.grad_clip_coef(a.grad, grad_scale, self.grad_max_norm) if self.grad_max_norm > 0 else None
        self.adam(grad_scale, self.nonfinite, grad_max_val=self.grad_max_val, clip_coef=coef, **hygiene)
        a.bump()


class _SideTable(_AdamState):
    """A small table of per-image parameters that MipTrainer trains beside the model, with an Adam of its own: `flat` with a gradient
    buffer `grad` and the moments in its layout.  Dense over the whole table like torch.optim.Adam: an entry visited earlier keeps
    moving on its momentum, an entry never visited has m = v = 0 and stays put exactly.  The module must stay where the trainer put it:
    a later `.to(...)` / `.float()` that reallocates its parameters would cut them off from `flat` (`check_views` raises then, before a
    step trains a table the module no longer sees).  A table supplies `ws_need` (its gradient kernel's fp64 scratch for n rays) and,
    where a rank needs more of it than `flat`, `broadcast_tensors`."""

    def _table_buffers(self, lr, betas, eps):
        self.grad, self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.lr, self.betas, self.eps, self.t = float(lr), tuple(betas), float(eps), 0
        self._ws = None

    def _buffers(self):
        return self.flat, self.grad

    def check_views(self):
        for n, lo, _, _ in self._layout():
            if getattr(self.net, n).data_ptr() != self.flat.data_ptr() + 4 * lo:
                raise RuntimeError(f"{self.what}: the module's {n} no longer lives in the trainer's flat {self.what} buffer (was the module moved or "
                                   "cast after MipTrainer took it?)")

    def broadcast_tensors(self):
        return [self.flat]

    def workspace(self, n):
        """fp64 scratch of the table's gradient kernel for n rays, kept between steps"""
        need = self.ws_need(n)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.float64, device=self.flat.device)
        return self._ws

    def train(self, world, group, nonfinite):
        """the table's Adam step (after the model's): the ranks' table gradients are summed like the model's, 1 / world folded in"""
        if world > 1:
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)
        self.t += 1
        self.adam(1.0 / world, nonfinite)


class _PoseFlat:
    """The flat pose table of a trainer: the trained parameters of a LearnPose / LearnPoseV2 -- `r`, then `t` when it is trained -- moved
    into one flat fp32 buffer (the module's parameters become views of it, so `pose_net.state_dict()` / `load_state_dict()` keep
    working).  `_flatten` allocates `flat`; `_adopt`, once the gradient buffer stands, moves the parameters in and cuts `g`."""
    what = "pose"

    def _flatten(self, pose_net, device):
        self.net = pose_net
        pose_net.to(device)
        self.shape = (pose_net.num_cams, 3)         # of every trained parameter
        self.names = [n for n in ("r", "t") if getattr(pose_net, n).requires_grad]
        if not self.names:
            raise ValueError("pose_net: neither r nor t is trained (learn_R / learn_t)")
        for n in ("r", "t"):
            p = getattr(pose_net, n)
            if p.dtype != torch.float32 or tuple(p.shape) != (pose_net.num_cams, 3):
                raise ValueError(f"pose_net.{n}: fp32 [num_cams, 3] expected")
        k = 3 * pose_net.num_cams
        self.flat = torch.zeros(k * len(self.names), dtype=torch.float32, device=device)

    def _adopt(self):
        k = 3 * self.net.num_cams
        self.g = {}
        for i, n in enumerate(self.names):
            p = getattr(self.net, n)
            view = self.flat[i * k:(i + 1) * k].view(-1, 3)
            view.copy_(p.data)
            p.data = view
            self.g[n] = self.grad[i * k:(i + 1) * k].view(-1, 3)

    def _layout(self):
        k = 3 * self.net.num_cams
        return [(n, i * k, k, self.shape) for i, n in enumerate(self.names)]

    def broadcast_tensors(self):
        """the whole table: an untrained t (learn_t=False) is applied to the rays all the same"""
        return [self.net.r.data, self.net.t.data]


class _PoseAdam(_PoseFlat, _SideTable):
    """The learned camera poses of a trainer (poses.LearnPose) and their Adam (utils/model_utils.py:36-42: its own optimiser, lr 1e-4) on
    the device, over the flat table of _PoseFlat.  State in the layout of
    torch.optim.Adam([{'params': [...], 'lr': 1e-4}]).state_dict(): the `optimizer` entry of the reference's pose/NNNNNN.tar."""

    def __init__(self, pose_net, device, lr, betas, eps):
        self._flatten(pose_net, device)
        self._table_buffers(lr, betas, eps)
        self._adopt()

    def ws_need(self, n):
        return ops.pose_grad_ws(n)


class _PoseSGD(_PoseFlat, _SideTable):
    """The per-ray learned poses of ZipTrainer (poses.LearnPoseV2) and their optimiser, plain SGD (s-nerfpp/zipnerf/internal/
    train_utils.py:290: torch.optim.SGD(posenet.parameters(), lr), stepped after clip_gradients(posenet), train.py:343) on the device:
    the flat table, its gradient buffer, no moments.  `lr` is a plain attribute read at step time: the caller applies the schedule
    (pn_lr_fn, train.py:181-183) by assigning it.  State in the layout of torch.optim.SGD([...], lr).state_dict()."""

    def __init__(self, pose_net, device, lr):
        self._flatten(pose_net, device)
        self.grad, self.lr, self._ws = torch.zeros_like(self.flat), float(lr), None
        self._adopt()

    def ws_need(self, n):
        return ops.pose_rays_grad_ws(n, self.net.num_cams)

    def train(self, world, group, nonfinite, loss_scale=1.0, grad_max_val=0.0, grad_max_norm=0.0, dropped=None):
        """the table's SGD step (after the model's update): the ranks' gradients are summed like the model's; the launch undoes the loss
        scale, takes the data-parallel mean, applies the trainer's gradient hygiene (train.py:343 clips the posenet with the model's
        config) and zeroes the gradient"""
        if world > 1:
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)
        scale = 1.0 / (world * loss_scale)
        coef = ops.grad_clip_coef(self.grad, scale, grad_max_norm) if grad_max_norm > 0 else None
        ops.sgd_step(self.flat, self.grad, self.lr, grad_scale=scale, nonfinite=nonfinite, grad_max_val=grad_max_val, clip_coef=coef, dropped=dropped)

    def _torch_sgd(self):
        return torch.optim.SGD([torch.nn.Parameter(torch.zeros(shape)) for *_, shape in self._layout()], lr=self.lr)

    def state_dict(self):
        return self._torch_sgd().state_dict()

    def load_state_dict(self, sd):
        """takes the learning rate; refuses, before it writes, a state for another number of parameters or an SGD this launch is not
        (momentum, dampening, weight decay, nesterov, maximize)"""
        groups = sd["param_groups"]
        if sum(len(g["params"]) for g in groups) != len(self._layout()):
            raise ValueError(f"pose optimizer state for {sum(len(g['params']) for g in groups)} parameters, {len(self._layout())} expected "
                             f"({', '.join(self.names)})")
        if any(float(g["lr"]) != float(groups[0]["lr"]) for g in groups[1:]):
            raise ValueError("the SGD launch covers the pose parameters with one lr: the saved param_groups differ")
        if any(float(g.get(k, 0) or 0) != 0 for g in groups for k in ("momentum", "dampening", "weight_decay")) or \
                any(g.get(k, False) for g in groups for k in ("nesterov", "maximize")):
            raise ValueError("the pose optimizer is plain SGD: no momentum / dampening / weight decay / nesterov / maximize")
        self._torch_sgd().load_state_dict(sd)          # (torch's own checks of the layout)
        self.lr = float(groups[0]["lr"])


class _ConfAdam(_SideTable):
    """The learned depth confidence of a trainer (confidence.Confidence + confidence.ConfidenceMaps) and its Adam (model/confidence.py:182-184:
    its own optimiser, lr 1e-3) on the device: the flat buffer is `lambdas` itself (moved to the device once).  State in the layout of
    torch.optim.Adam([{'params': [lambdas], 'lr': 1e-3}]).state_dict(): the `optimizer_conf` entry of the reference's checkpoint."""
    what = "confidence"

    def __init__(self, conf_net, maps, device, lr, betas, eps):
        self.net = conf_net
        conf_net.to(device)
        p = conf_net.lambdas
        if p.dtype != torch.float32 or p.dim() != 2 or not p.requires_grad:
            raise ValueError("conf_net.lambdas: a trained fp32 [n_modes, n_images] table expected")
        p.data = p.data.contiguous()
        self.maps = maps.for_model(conf_net).to(device)
        self.names, self.shape = ["lambdas"], tuple(p.shape)
        self.flat = p.data.view(-1)
        self._table_buffers(lr, betas, eps)
        self.g = self.grad.view(p.shape)

    def _layout(self):
        return [("lambdas", 0, self.flat.numel(), self.shape)]

    def ws_need(self, n):
        return ops.conf_grad_ws(n)

    def apply(self, img, coords):
        """-> the confidence of the rays at pixels coords of image img, [n]"""
        m = self.maps
        return ops.conf_apply(m.maps, m.slot_of_image, self.net.lambdas.data, m.sky, img, coords)

    def reduce(self, img, coords, g_conf):
        """d loss / d conf [n] into the gradient buffer's column of image img"""
        m = self.maps
        ops.conf_grad(m.maps, m.slot_of_image, self.net.lambdas.data, m.sky, img, coords, g_conf, self.g, ws=self.workspace(coords.shape[0]))



class MipLossRules:
    """The per-image rules of the reference's loss block (s-nerf/train.py:131-209) as three int32 tables with one entry per image, built
    once; the loss tail looks up the entry of the batch's image on the device (ops.mip_loss_tail_masked), so the step never reads the
    image index on the host.
      rgb_row_limit[i]    rays of pixel rows >= it leave the RGB and the semantic mean: `waymo_row_limit` where `waymo` is set and
                          camera_index[i] is one of `waymo_cams` (train.py:137-144: --waymo, cameras 3 and 4, row 886), else H (no rule)
      depth_row_limit[i]  rays of rows >= it leave the depth mean: `backcam_row_limit` where `backcam` is set and camera_index[i] ==
                          `backcam_cam` (train.py:165-170, loss.py:344-346: --backcam, camera 0, row 750), else H
      sem_valid[i]        1 for the images of `semantic_index` (train.py:131,185: the images with labels), else 0: no semantic term
    `camera_index`: the camera of every image ([num_images], as the reference's cam_index).  The tables are host tensors;
    `on(device)` returns (and keeps) their device copies."""

    def __init__(self, num_images, H, camera_index, semantic_index=None, waymo=False, backcam=False, waymo_cams=(3, 4), waymo_row_limit=886,
                 backcam_cam=0, backcam_row_limit=750):
        import numpy as np
        n = int(num_images)
        cam = np.asarray(camera_index.cpu() if torch.is_tensor(camera_index) else camera_index).reshape(-1)
        if n < 1 or cam.shape[0] != n:
            raise ValueError(f"MipLossRules: camera_index needs one entry per image ({n}), got {cam.shape[0]}")
        rgb = np.full(n, int(H), np.int32)
        dep = np.full(n, int(H), np.int32)
        sem = np.zeros(n, np.int32)
        if waymo:
            rgb[np.isin(cam, list(waymo_cams))] = int(waymo_row_limit)
        if backcam:
            dep[cam == backcam_cam] = int(backcam_row_limit)
        if semantic_index is not None:
            idx = np.asarray(semantic_index.cpu() if torch.is_tensor(semantic_index) else list(semantic_index), dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= n):
                raise ValueError("MipLossRules: semantic_index points past the images")
            sem[idx] = 1
        self.num_images, self.H = n, int(H)
        self.rgb_row_limit, self.depth_row_limit, self.sem_valid = torch.from_numpy(rgb), torch.from_numpy(dep), torch.from_numpy(sem)
        self._dev = {}

    def on(self, device):
        """-> (rgb_row_limit, depth_row_limit, sem_valid) on `device`"""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.rgb_row_limit, self.depth_row_limit, self.sem_valid))
        return self._dev[key]


class MipTrainer(_CapturedStep, _ArenaAdam):
    rules = None                                     # (class default: loss_and_grads also serves trainers assembled without __init__)
    smooth_patch_sz = None

    def __init__(self, model, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, depth_lambda=0.2, coarse_depth_mult=0.2,
                 proposal_loss=False, proposal_lambda=0.05, disparity_depth=True, process_group=None,
                 nonfinite="zero", grad_max_val=0.0, grad_max_norm=0.0, exchange_when_single=False,
                 pose_net=None, pose_lr=1e-4, pose_betas=(0.9, 0.999), pose_eps=1e-8, semantic_lambda=0.1, loss_rules=None,
                 conf_net=None, conf_maps=None, conf_lr=1e-3, conf_betas=(0.9, 0.999), conf_eps=1e-8,
                 smooth_patch_sz=None, smooth_lambda=0.1, smooth_skymask=True, freeze_model=False, pose_compose=False):
        """`nonfinite` / `grad_max_val` / `grad_max_norm`: gradient hygiene folded into the Adam launch (ops.adam_step).  The s-nerf
        reference has none (train.py:212-215 drops into pdb on a failing backward); the default "zero" keeps one NaN / Inf gradient
        (1/(depth + eps), a bf16 overflow) from poisoning m, v and the parameters of the whole arena on every rank.  "keep" = plain Adam.
        `pose_net` (poses.LearnPose; configs: pose_refine = True): the learned camera poses are trained inside the step -- see `step`'s
        `img_i`.  The module is moved to the model's device and its trained parameters into one flat buffer (`self.pose`, _PoseAdam);
        `pose_lr` / `pose_betas` / `pose_eps`: their own Adam (utils/model_utils.py:36-42: lr 1e-4, no schedule).
        `semantic_lambda` (arg_parser.py:166): weight of the semantic cross-entropy of `step`'s `target_semantic`.  `loss_rules`
        (MipLossRules): the Waymo side-camera / back-camera masks and the images with labels, applied inside the loss tail to the image
        `step`'s `img_i` names.
        `conf_net` + `conf_maps` (confidence.Confidence / ConfidenceMaps; configs: depth_conf = True, precompute_conf = True): the
        per-ray depth confidence is mixed from the precomputed maps with the learned per-image weights and those are trained inside
        the step (`self.conf`, _ConfAdam) -- see `step`.  `conf_lr` / `conf_betas` / `conf_eps`: their own Adam (confidence.py:182-184:
        lr 1e-3, no schedule).
        `smooth_patch_sz` (configs: smooth_loss = True; arg_parser's patch_sz; None = off): the edge-aware smoothness of depth patches
        (train.py:154-177) joins the step -- see `step`'s `n_rgb`.  `smooth_lambda`: its weight (arg_parser's smooth_lambda);
        `smooth_skymask`: edges whose left / top pixel is sky count twice (SmoothLoss's use_skymask), `step` then needs `smooth_sky`.
        `freeze_model` (needs a `pose_net`; the reference's test-time pose refinement, eval.py:77-114, --test_refine_iter): the network is
        held fixed and only the side tables are trained -- the step is pose apply, forward, loss tail, the backward's data path alone
        (MipNerfModel._backward(ray_grads=True, weight_grads=False): no weight-gradient GEMM, no bias-gradient sums), the pose gradient and
        the side tables' Adam; no gradient exchange of the arena, no arena Adam, `self.t` / `self.m` / `self.v` and the arena stay as
        they are.  world > 1: the pose gradient is still summed over the ranks.
        `pose_compose` (with a `pose_net`): the table row is COMPOSED with the initial pose as eval.py:88-89 does
        (make_c2w(r, t) @ init_c2w[img]) -- on the rays of the initial pose o' = R o + t, d' = R d (ops.pose_compose_apply /
        ops.pose_compose_grad) -- where the training-time route (sample_utils.py:421-435) shifts the origins without turning them."""
        if freeze_model and pose_net is None:
            raise ValueError("MipTrainer: freeze_model=True trains the pose table alone: it needs pose_net=")
        if pose_compose and pose_net is None:
            raise ValueError("MipTrainer: pose_compose=True needs pose_net= (the table whose rows are composed with the rays' initial pose)")
        self.freeze_model, self.pose_compose = bool(freeze_model), bool(pose_compose)
        self._arena_buffers(model, lr, betas, eps, nonfinite, grad_max_val, grad_max_norm, process_group)
        self.depth_lambda, self.coarse_depth_mult = depth_lambda, coarse_depth_mult
        self.proposal_loss, self.proposal_lambda, self.disparity_depth = proposal_loss, proposal_lambda, disparity_depth
        a = model.arena
        self.single_rank_exchange = bool(exchange_when_single) and dist.is_available() and dist.is_initialized()
        self.pose = None if pose_net is None else _PoseAdam(pose_net, a.flat.device, pose_lr, pose_betas, pose_eps)
        self.semantic_lambda, self.rules = float(semantic_lambda), loss_rules
        self._rule_tables = None if loss_rules is None else loss_rules.on(a.flat.device)
        self.last_semantic_loss = self.last_counts = None
        self._img_dev = None                         # (python int img_i, its int64 [1] device tensor)
        if (conf_net is None) != (conf_maps is None):
            raise ValueError("MipTrainer: conf_net= and conf_maps= go together (the learned weights and the maps they mix)")
        self.conf = None if conf_net is None else _ConfAdam(conf_net, conf_maps, a.flat.device, conf_lr, conf_betas, conf_eps)
        self.side = [x for x in (self.pose, self.conf) if x is not None]      # the side tables there are, in the order of their Adam launches
        self.smooth_patch_sz = None if smooth_patch_sz is None else int(smooth_patch_sz)
        if self.smooth_patch_sz is not None and not 2 <= self.smooth_patch_sz <= 32:
            raise ValueError("MipTrainer: smooth_patch_sz in 2..32 (one workgroup lane per patch pixel)")
        self.smooth_lambda, self.smooth_skymask = float(smooth_lambda), bool(smooth_skymask)
        self.last_smooth_loss = None
        self._smooth_bufs = {}                       # the trainer's own depth targets / labels / scratch of the smooth term, by shape

    def pose_state_dict(self):
        """the pose optimiser's state in torch.optim.Adam's layout (the `optimizer` entry of the reference's pose/NNNNNN.tar; the table
        itself is `pose_net.state_dict()`, its `model_param` entry)"""
        return self.pose.state_dict()

    def load_pose_state_dict(self, sd):
        self.pose.load_state_dict(sd)

    def conf_state_dict(self):
        """the confidence optimiser's state in torch.optim.Adam's layout (the `optimizer_conf` entry of the reference's checkpoint; the
        table itself is `conf_net.state_dict()`, its `confidence` entry)"""
        return self.conf.state_dict()

    def load_conf_state_dict(self, sd):
        self.conf.load_state_dict(sd)

    def _trained(self):
        """what the step's Adam launches train, in their order: the arena (unless the model is frozen), then the side tables"""
        return ([] if self.freeze_model else [self]) + self.side

    def _update(self):
        """the model's Adam (unless it is frozen), then the side tables'; graph mode: step counts and learning rates live on the device
        (capture / replay below)"""
        if not self.freeze_model:
            self.t += 1
            self._arena_adam(1.0 / self.world)
        for table in self.side:
            table.train(self.world, self.pg, self.nonfinite)

    def loss_and_grads(self, outs, target_rgb, target_depth, conf, target_semantic=None, sel_coords=None, img_i=None, depth_keep=None,
                       want_g_conf=False):
        """The reference's per-ray loss tail (train.py:150-208) in ONE kernel, `snerf_mip_loss_tail`: RGB MSE, the
        confidence-weighted (disparity) depth loss on both levels masked to rays with a LiDAR target, and -- with
        `proposal_loss` -- ProposalLoss on the two histograms.  Returns (loss [device scalar], output gradients).
        With `target_semantic`, `depth_keep` or loss rules (see `step`): `snerf_mip_loss_tail_masked`, which adds the semantic
        cross-entropy and the per-image masks of train.py:131-209; the output gradients then end with g_semantic.  `last_losses` keeps
        its four entries; `last_semantic_loss` and `last_counts` = (#depth rays, #rgb rays, #semantic rays) are device scalars too.
        `want_g_conf` (the learned confidence): the masked tail's g_conf route; `last_g_conf` [n] = d loss / d conf."""
        dist0, acc0, s0, w0, rgb1, dist1, acc1, s1, w1 = outs[:9]
        rules = self.rules
        dist1, dist0 = (dist1, dist0) if target_depth is not None else (None, None)
        hists = (s1, w1, s0, w0) if self.proposal_loss else (None, None, None, None)
        args = (rgb1, target_rgb, dist1, dist0, target_depth, conf, *hists, self.disparity_depth, self.depth_lambda, self.coarse_depth_mult,
                self.proposal_lambda)
        if target_semantic is not None or depth_keep is not None or rules is not None or want_g_conf:
            tables = self._rule_tables if rules is not None else (None, None, None)
            with_sem = target_semantic is not None
            out, g_rgb1, g_dist1, g_dist0, g_w0, g_sem, *g_conf = ops.mip_loss_tail_masked(
                *args, sem=outs[9] if with_sem else None, labels=target_semantic, semantic_lambda=self.semantic_lambda,
                rows=sel_coords if rules is not None else None, img_i=img_i if rules is not None else None,
                rgb_row_limit=tables[0], depth_row_limit=tables[1], sem_valid=tables[2], depth_keep=depth_keep,
                **(dict(want_g_conf=True) if want_g_conf else {}))
            self.last_g_conf = g_conf[0] if want_g_conf else None
            self.last_losses = out[:4]
            self.last_semantic_loss, self.last_counts = out[5], (out[0], out[6], out[7])
            return out[4], (g_dist0, None, g_w0, g_rgb1, g_dist1, None, None, g_sem)
        out, g_rgb1, g_dist1, g_dist0, g_w0 = ops.mip_loss_tail(*args)
        self.last_losses = out[:4]                               # {#valid depth rays, rgb, depth, proposal}: stays on the device
        return out[4], (g_dist0, None, g_w0, g_rgb1, g_dist1, None, None)      # out[4]: their sum, formed by the same launch

    def step(self, rays, target_rgb, target_depth=None, conf=None, randomized=True, s_rand=None, u=None, ray_grads=False, viewc=None, img_i=None,
             target_semantic=None, sel_coords=None, depth_keep=None, n_rgb=None, smooth_sky=None):
        """`ray_grads=True` (pose refinement, configs: pose_refine = True): `last_ray_grads` = d loss / d (origins, directions, viewdirs)
        of this rank's rays, for the caller's pose optimiser (`rays.origins.backward(g_o)` etc. chains them into the pose parameters).
        `viewc` (fn = 0 models, the view-centred warp): the warp centre the reference passes to every forward (train.py:36,112); a model
        built with fn = 0 refuses to step until a centre has been given here or through `model.set_viewc`.
        With a `pose_net`: `rays` are the UNtransformed rays of image `img_i` (a python int, or the batcher's int64 [1] device tensor,
        which is never read on the host); the step applies row img_i of the pose table to them (ops.pose_apply: sample_rays' pose
        branch), runs forward, loss tail and backward with ray gradients (`last_ray_grads` as above), reduces those to the row's gradient
        (ops.pose_grad) and follows the model's Adam with the pose table's -- no torch op, autograd graph or host sync in between.
        With `pose_compose` the row is composed with the rays' initial pose instead (ops.pose_compose_apply / ops.pose_compose_grad:
        o' = R o + t); with `freeze_model` the backward forms no weight gradient and the model's Adam is left out (see __init__).
        `target_semantic` (a model with semantic=True): per-ray labels, int32 or fp32 holding exact integers (a batcher's extras row;
        other integer types are converted), -100 = ignored; the semantic cross-entropy times `semantic_lambda` joins the loss and
        trains the semantic head (train.py:185-191).  A label outside [0, C) other than -100 is ignored as well -- the reference
        raises on one.  `depth_keep` [n] fp32 (with target_depth): a ray counts for the depth term only where it is 0 (train.py:168-170,
        seg_mask == 0).  With `loss_rules`: `sel_coords` (the batcher's int64 [n,2] pixel coordinates) and `img_i` (as above; a
        python int is wrapped into a device tensor once per value) are needed, and the tail applies the rules of that image: rays of pixel rows at or past
        the RGB row limit leave the RGB and semantic means, rays at or past the depth row limit (or with depth_keep != 0) the depth mean
        -- and, as in the reference, only that one -- and images outside the rules' semantic_index have no semantic term.  A term that counts
        no ray is 0 with zero gradients, where the reference's empty mean is NaN.  world > 1: every rank forms its means over its
        own shard of the batch, like the reference under DDP and like the depth term's count before.
        With a `conf_net`: `target_depth`, `sel_coords` and `img_i` are needed and `conf=` is refused; the step mixes the confidence of
        the batch's rays from the maps with the learned weights of image img_i (ops.conf_apply, never a host read of the index), runs
        the loss tail's g_conf route (loss rules, `depth_keep` and the semantic term keep working), reduces d loss / d conf to the
        gradient of the image's column of the table right behind the tail (ops.conf_grad) and follows the model's Adam (and the pose
        table's) with the confidence table's.  `last_conf` [n] is the confidence the step used.
        With `smooth_patch_sz` = p (train.py:149-191): `n_rgb` = the number of rows in front of the batch's patch rows (a
        PatchRayBatcher's `n_rgb_rows`); the n - n_rgb rows behind them are whole patches of p^2 rays each, so their number is read from
        the batch and a rank's share needs no other plumbing.  The RGB and proposal terms count all n rays; the depth terms and the
        semantic term count the first n_rgb only: the tail is handed a depth target of 0 (what it masks out already; calc_depth_loss
        averages over target_depth != 0, so this equals the reference's slicing) and a label of -100 on the patch rows, in buffers the
        trainer owns -- the caller's tensors are never written.  Behind the tail, ops.smooth_loss runs on target_rgb[n_rgb:] and the
        fine distances [n_rgb:] and adds smooth_lambda * SmoothLoss to the loss and its gradient to the fine level's distance
        gradient.  `smooth_sky` fp32 [n - n_rgb] (the batcher's sky extra on the patch rows): needed iff `smooth_skymask`.
        `last_smooth_loss` is a device scalar; `last_losses` keeps its four entries.  A batch without patch rows (n_rgb == n) launches
        nothing more and the term is 0.  world > 1: every rank averages over its own patches, like the other terms.  The reference
        slices the semantic rows AFTER its Waymo row mask (train.py:142-144,186-187), which misaligns labels and rays; that is not
        reproduced: the semantic term counts the first n_rgb rays that pass the rules."""
        self._set_viewc(viewc)
        if self.pose is not None and img_i is None:
            raise ValueError("MipTrainer with a pose_net: step() needs img_i= (the image the rays belong to)")
        if self.pose is None and self.rules is None and self.conf is None and img_i is not None:
            raise ValueError("MipTrainer: img_i= given without a pose_net or loss_rules")
        if self.conf is not None:
            if conf is not None:
                raise ValueError("MipTrainer with a conf_net: the step forms the confidence itself, conf= cannot be given")
            if target_depth is None or sel_coords is None or img_i is None:
                raise ValueError("MipTrainer with a conf_net: step() needs target_depth=, sel_coords= and img_i= (the confidence weighs the depth term "
                                 "of the batch's pixels with the weights of its image)")
        # every block of the gradient arena goes on the wire as soon as the backward pass has finished it (heads, then trunk layer by
        # trunk layer, then the proposal network): the collectives run under the remaining backward kernels.  A frozen model has no
        # arena gradient to exchange (the side tables' gradients are summed by _SideTable.train)
        ex = None if self.freeze_model else _GradExchange(self.model.arena, self.world, self.pg, self.single_rank_exchange)
        loss, outs = self._forward_backward(rays, target_rgb, target_depth, conf, randomized, s_rand, u, ray_grads, ex, img_i,
                                            target_semantic, sel_coords, depth_keep, n_rgb, smooth_sky)
        if ex is not None:
            ex.finish()
        self._update()
        return loss, outs

    def _set_viewc(self, viewc):
        m = self.model
        if viewc is not None:
            m.set_viewc(viewc)
        elif m.fn == 0 and not getattr(m, "_viewc_given", False):
            raise ValueError("MipTrainer: the model warps around a view centre (fn = 0): pass viewc= (train.py:36,112) or call model.set_viewc first")

    def _batch_index(self, n, dev, img_i, sel_coords):
        """the batch's image and pixels in the forms the step's kernels take -> (img, img_dev, coords): `img` for the pose and confidence
        kernels (a python int stays one, a device tensor is never read on the host), `img_dev` for the rules of the loss tail (always a
        device tensor), `coords` int64 [n, 2] on the device where the confidence or the rules look pixels up, else None"""
        indexed = self.rules is not None or self.conf is not None
        if self.rules is not None and (sel_coords is None or img_i is None):
            raise ValueError("MipTrainer with loss_rules: step() needs sel_coords= and img_i= (the pixels and the image of the batch)")
        img = img_dev = coords = None
        if torch.is_tensor(img_i):
            img = img_dev = img_i.to(dev)
        elif img_i is not None:
            img = int(img_i)
            if self.rules is not None:                   # wrapped once per value: steps on the same image upload nothing
                if self._img_dev is None or self._img_dev[0] != img:
                    self._img_dev = (img, torch.tensor([img], dtype=torch.int64, device=dev))
                img_dev = self._img_dev[1]
        if indexed:
            coords = sel_coords.to(dev, torch.int64).contiguous()
            if tuple(coords.shape) != (n, 2):
                raise ValueError("MipTrainer: sel_coords is the batcher's [n, 2] (row, col) per ray")
        return img, img_dev, coords

    def _tail_extras(self, n, dev, target_depth, target_semantic, depth_keep):
        """checks and device forms of the masked tail's per-ray inputs -> (target_semantic, depth_keep)"""
        if target_semantic is not None:
            if not getattr(self.model, "semantic", False):
                raise ValueError("MipTrainer: target_semantic= given, but the model has no semantic head (semantic=True)")
            if self.rules is not None and not bool(self.rules.sem_valid.any()):
                raise ValueError("MipTrainer: target_semantic= given, but the loss rules name no image with labels (semantic_index)")
            if target_semantic.dtype not in (torch.int32, torch.float32):
                target_semantic = target_semantic.to(torch.int32)
            target_semantic = target_semantic.to(dev).reshape(-1).contiguous()
            if target_semantic.shape[0] != n:
                raise ValueError("MipTrainer: target_semantic needs one label per ray")
        if depth_keep is not None:
            if target_depth is None:
                raise ValueError("MipTrainer: depth_keep= masks the depth term: it needs target_depth=")
            depth_keep = depth_keep.to(dev, torch.float32).reshape(-1).contiguous()
        return target_semantic, depth_keep

    def _smooth_own(self, key, src, n_rgb, fill):
        """the trainer's own copy of a per-ray target whose patch rows [n_rgb:] hold `fill` (set once, when the buffer is made); one
        copy launch per step, the caller's tensor is only read"""
        key = (key, tuple(src.shape), src.dtype, n_rgb)
        own = self._smooth_bufs.get(key)
        if own is None:
            own = self._smooth_bufs[key] = torch.full_like(src, fill)
        own[:n_rgb].copy_(src[:n_rgb])
        return own

    def _smooth_split(self, n, n_rgb, smooth_sky, dev):
        """checks of step's smooth arguments -> (n_rgb, number of patches, sky [P p^2] or None)"""
        if self.smooth_patch_sz is None:
            if n_rgb is not None or smooth_sky is not None:
                raise ValueError("MipTrainer: n_rgb= / smooth_sky= given, but the smooth term is off (smooth_patch_sz=None)")
            return n, 0, None
        if n_rgb is None:
            raise ValueError("MipTrainer with smooth_patch_sz: step() needs n_rgb= (the rows in front of the patch rows; a PatchRayBatcher's n_rgb_rows)")
        n_rgb, pp = int(n_rgb), self.smooth_patch_sz ** 2
        if not 0 <= n_rgb <= n or (n - n_rgb) % pp:
            raise ValueError(f"MipTrainer: the {n} - n_rgb = {n - n_rgb} patch rows are not whole patches of {pp} rays")
        if self.smooth_skymask != (smooth_sky is not None):
            raise ValueError("MipTrainer: smooth_sky= (the sky mask on the patch rows) is needed with smooth_skymask=True and only then")
        if smooth_sky is not None:
            smooth_sky = smooth_sky.to(dev, torch.float32).reshape(-1).contiguous()
            if smooth_sky.shape[0] != n - n_rgb:
                raise ValueError("MipTrainer: smooth_sky needs one value per patch row")
        return n_rgb, (n - n_rgb) // pp, smooth_sky

    def _smooth_term(self, outs, target_rgb, n_rgb, P, sky, loss, g):
        """ops.smooth_loss behind the tail: the loss joins the tail's total (`loss` is that device word), the gradient the fine level's
        distance gradient -> g with g_dist1 in place"""
        dist1 = outs[5].reshape(-1)
        g_dist1, fresh = g[4], g[4] is None
        if fresh:                                        # (no depth term: the tail formed no distance gradient)
            g_dist1 = torch.zeros_like(dist1)
        ws = self._smooth_bufs.get(("ws", P))
        if ws is None:
            ws = self._smooth_bufs[("ws", P)] = torch.empty(ops.smooth_loss_ws(P), dtype=torch.float64, device=dist1.device)
        out = torch.empty(3, dtype=torch.float32, device=dist1.device)
        ops.smooth_loss(target_rgb[n_rgb:], dist1[n_rgb:], sky, P, self.smooth_patch_sz, self.smooth_lambda, out=out, total=loss,
                        g_dist=g_dist1.reshape(-1)[n_rgb:], accumulate=not fresh, ws=ws)
        self.last_smooth_loss = out[0]
        return g[:4] + (g_dist1,) + g[5:]

    def _forward_backward(self, rays, target_rgb, target_depth, conf, randomized, s_rand, u, ray_grads, on_done, img_i=None,
                          target_semantic=None, sel_coords=None, depth_keep=None, n_rgb=None, smooth_sky=None):
        """draws, both levels forward, the fused loss tail, the backward pass into the gradient arena (no exchange, no optimiser); with a
        pose table: its row applied to the rays in front, the ray gradients reduced into its gradient buffer behind"""
        m = self.model
        dev = m.arena.flat.device
        n = rays.origins.shape[0]
        ps = self.pose
        cf = self.conf
        n_rgb, n_patches, smooth_sky = self._smooth_split(n, n_rgb, smooth_sky, dev)
        for table in self.side:
            table.check_views()
        img, img_dev, coords = self._batch_index(n, dev, img_i, sel_coords)
        if cf is not None:
            conf = self.last_conf = cf.apply(img, coords)
        target_semantic, depth_keep = self._tail_extras(n, dev, target_depth, target_semantic, depth_keep)
        if n_patches > 0:                                # the depth and semantic terms leave the patch rows out
            if target_depth is not None:
                target_depth = self._smooth_own("depth", target_depth, n_rgb, 0.0)
            if target_semantic is not None:
                target_semantic = self._smooth_own("labels", target_semantic, n_rgb, -100)
        if ps is not None:
            f32 = lambda x: x.detach().to(dev, torch.float32).contiguous()
            o, d, v = f32(rays.origins), f32(rays.directions), f32(rays.viewdirs)
            apply = ops.pose_compose_apply if self.pose_compose else ops.pose_apply
            rays = rays._replace(**dict(zip(("origins", "directions", "viewdirs"), apply(ps.net.r.data, ps.net.t.data, img, o, d, v))))
            ray_grads = True
        ds_rand, du, noise0, noise1 = m._draws(n, randomized, dev)
        s_rand = ds_rand if s_rand is None else s_rand
        u = du if u is None else u
        outs, ctx = m._run(rays, True, False, s_rand, u.contiguous(), noise0, noise1)
        loss, g = self.loss_and_grads(outs, target_rgb, target_depth, conf, target_semantic, coords, img_dev, depth_keep, want_g_conf=cf is not None)
        if cf is not None:
            cf.reduce(img, coords, self.last_g_conf)
        if n_patches > 0:
            g = self._smooth_term(outs, target_rgb, n_rgb, n_patches, smooth_sky, loss, g)
        elif self.smooth_patch_sz is not None:
            self.last_smooth_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.last_ray_grads = m._backward(ctx, *g, on_done=on_done, ray_grads=ray_grads, weight_grads=not self.freeze_model)
        if ps is not None:
            g_o, g_d, g_v = self.last_ray_grads
            if self.pose_compose:                        # (the rotation reached the origins: the untransformed ones join the reduction)
                ops.pose_compose_grad(ps.net.r.data, img, g_o, g_d, g_v, o, d, v, ps.g.get("r"), ps.g.get("t"), ws=ps.workspace(n))
            else:
                ops.pose_grad(ps.net.r.data, img, g_o, g_d, g_v, d, v, ps.g.get("r"), ps.g.get("t"), ws=ps.workspace(n))
        return loss, outs

    # ---- hipGraph capture of the whole step --------------------------------------------------------------------------------------
    def capture(self, rays, target_rgb, target_depth=None, conf=None, randomized=True, warmup=3, viewc=None, batcher=None, conf_extra=None,
                img_i=None, sem_extra=None, depth_keep_extra=None, smooth_sky_extra=None):
        """Capture one full training step (draws, forward, loss tail, backward, Adam: ~130 launches) in a hipGraph over the GIVEN tensors;
        afterwards `replay()` runs a step with one graph launch -- the caller refreshes the batch by copying into those tensors
        (`rays.origins.copy_(...)` etc.).  Worth it when the step is launch-bound: at 512 rays per GPU (the 8-GPU split of the
        reference's 4096-ray batch) the kernels are 10-50 us each.  The packed-weight refresh, the torch RNG draws (graph-safe Philox
        offsets), the Adam bias corrections (step count in device memory) and the learning rate (device scalar, refreshed from
        `self.lr` by every `replay()`, so an lr schedule keeps working) are all inside the graph.

        The `warmup` steps (one-time kernel attributes, allocator pools) are REAL steps on the capture batch, so parameters, Adam
        moments and the step count are snapshotted before and restored after them: capturing does not train.  (The torch RNG does
        advance.)

        Data parallel (world > 1; every rank calls capture / replay together): the graph holds forward + loss tail + backward -- the
        launch-bound part -- and `replay()` follows it with the gradient all-reduce and the Adam launch OUTSIDE the graph (one
        collective over the whole arena: nothing is left to overlap it with once the backward is a single graph launch; the
        collective stays out of the graph so that any backend works, gloo on the 1-GPU box included).

        `batcher` (sample_utils.ImageRayBatcher): its draw (`next_into`, one launch) becomes the first node of the captured step, whose
        rays and targets are the batcher's buffers (`rays` / `target_rgb` / `target_depth` are ignored; `conf_extra` = index of the
        batcher's extra map that serves as the per-ray confidence, or None): every `replay()` trains on a fresh batch, the k-th on the
        batch an eager batcher draws at step s0 + k (s0 = the batcher's step at this call).  The warm-up restores the batcher's counter
        like the parameters.  `self.batch` holds the captured batch tensors (rays, target_rgb, target_depth, sel_coords, img_i, extras).

        With a `pose_net` the captured step is the draw, ops.pose_apply fed by the batch's `img` tensor (without a batcher: `img_i`, an
        int64 [1] device tensor the caller refreshes like the rays), forward, backward with ray gradients, ops.pose_grad and both Adams
        (world > 1: both Adams and the two all-reduces follow the graph); the pose table, its moments and step count are snapshotted and
        restored around the warm-up like the model's.  `pose_compose` swaps in ops.pose_compose_apply / ops.pose_compose_grad;
        `freeze_model`: the captured step ends with the side tables' Adam launches -- it holds no weight-gradient GEMM and no arena Adam
        node, and neither capture nor replay touches the arena, its moments or `self.t`.

        With a `conf_net` (batcher only; `conf_extra` stays None) the captured step also holds ops.conf_apply and ops.conf_grad, fed by the
        batch's `sel_coords` and `img` buffers, and the confidence table's Adam (world > 1: that Adam and its all-reduce follow the
        graph); the table, its moments and step count are snapshotted and restored around the warm-up like the pose table's.

        `sem_extra` / `depth_keep_extra`: indices of the batcher's extra maps that serve as `step`'s `target_semantic` (a label map
        stored as fp32) and `depth_keep` (a seg map); with loss rules the captured tail takes `sel_coords` and the image from the batch
        buffers, so every replay applies the rules of the image it drew, without a host read.  (Labels, `depth_keep` and loss rules
        are captured with a batcher only.)

        With `smooth_patch_sz` (a sample_utils.PatchRayBatcher only): the captured step takes `n_rgb` from the batcher's `n_rgb_rows`
        and, with `smooth_skymask`, the sky of the patch rows from the batcher's extra map `smooth_sky_extra`; the trainer-owned target
        copies, ops.smooth_loss and its finish launch are nodes of the graph.  Nothing on the host depends on the batch."""
        indexed = bool(self.side) or self.rules is not None
        buf = None
        # every refusal first: a refused capture leaves the trainer as it was
        if self.smooth_patch_sz is not None:
            if not getattr(batcher, "draws_patches", False) or batcher.patch_sz != self.smooth_patch_sz:
                raise ValueError("capture() with smooth_patch_sz needs batcher= a PatchRayBatcher of that patch size: the captured step takes "
                                 "the patch rows from its buffers")
            if self.smooth_skymask != (smooth_sky_extra is not None):
                raise ValueError("capture(): smooth_sky_extra= (the batcher's sky extra) is needed with smooth_skymask=True and only then")
        elif smooth_sky_extra is not None:
            raise ValueError("capture(): smooth_sky_extra= given, but the smooth term is off (smooth_patch_sz=None)")
        if self.rules is not None and batcher is None:
            raise ValueError("capture() with loss_rules needs batcher=: the captured tail takes sel_coords and the image from its buffers")
        if self.conf is not None and batcher is None:
            raise ValueError("capture() with a conf_net needs batcher=: the captured step takes sel_coords and the image from its buffers")
        tail = dict(target_semantic=None, sel_coords=None, depth_keep=None, n_rgb=None, smooth_sky=None)
        if batcher is not None:
            buf = batcher.buffers()
            batch = batcher.view(buf)
            rays, target_rgb, target_depth, coords, img, extras = batch
            extra = lambda i: None if i is None else extras[i]
            conf = extra(conf_extra)
            tail.update(target_semantic=extra(sem_extra), depth_keep=extra(depth_keep_extra))
            img_i = img if indexed else None
            if self.rules is not None or self.conf is not None:
                tail.update(sel_coords=coords)
            if self.smooth_patch_sz is not None:
                tail.update(n_rgb=batcher.n_rgb_rows, smooth_sky=None if smooth_sky_extra is None else extras[smooth_sky_extra][batcher.n_rgb_rows:])
        if indexed and not (torch.is_tensor(img_i) and img_i.is_cuda):
            raise ValueError("capture() with a pose_net or loss_rules: img_i= must be an int64 [1] device tensor (a python int would be frozen into the graph)")
        self._set_viewc(viewc)                           # (fn = 0: the centre is a kernel argument, i.e. a constant of the captured graph)
        if batcher is not None:
            self.batch = batch
        step = dict(rays=rays, target_rgb=target_rgb, target_depth=target_depth, conf=conf, randomized=randomized, img_i=img_i, **tail)
        return self._capture(warmup, batcher, buf, lambda: self.step(**step),
                             lambda: self._forward_backward(s_rand=None, u=None, ray_grads=False, on_done=None, **step))

    def _bump_restored(self):
        if not self.freeze_model:
            self.model.arena.bump()

    def _after_graph(self):
        if not self.freeze_model:
            _GradExchange(self.model.arena, self.world, self.pg).finish()   # one all-reduce of the flat gradient arena
        self._update()


class _TableShards:
    """Hash-table gradients without the dense all-reduce (the reference all-reduces the dense ~310 MB through DDP,
    zipnerf/train.py:334).  Touched-rows-only exchange does not apply at the reference's batch sizes -- a rank's 8 192 rays put 14.7 M
    multisample cells on every 2^21-row level: every row is touched -- so the table spans go the ZeRO-1 way instead: REDUCE-SCATTER of
    the gradient span (each rank receives the sum of its 1 / world slice), Adam on that slice only (its m / v slices; 1 / world of the
    optimiser pass), ALL-GATHER of the updated parameter slices.  Same bytes on the wire as the all-reduce it replaces (a ring all-reduce
    is exactly these two phases) with the optimiser work of the tables sharded; the MLP parameters keep the bucketed all-reduce.
    Level sizes are multiples of 8 rows (grid.py:130), so the spans divide evenly for world sizes 2 / 4 / 8; other world sizes, and
    global-norm clipping (which needs the norm of the whole reduced gradient), use the all-reduce path.  A rank's slice of a
    single-channel table is NOT a multiple of 4 floats at world 4 / 8 (6 606 952 / 8 = 825 869): ops.adam_step takes its four
    pointers at any 4-byte alignment (scalar flavour of the kernel; tests/test_gpu_kernels.py::test_adam_on_misaligned_slices...)."""

    def __init__(self, arena, names, world, group):
        self.arena, self.world, self.group = arena, world, group
        self.rank = dist.get_rank(group)
        self.spans = {}
        for n in names:
            a, b = arena.span(n)
            if (b - a) % world != 0:
                raise ValueError("table span does not divide by the world size")
            self.spans[n] = (a, b, (b - a) // world)
        self.nccl = dist.get_backend(group) == "nccl"
        self.pending = []

    def reduce_scatter(self, name):
        """start the reduce-scatter of one table's gradient span; -> nothing (finish() waits)"""
        a, b, per = self.spans[name]
        g = self.arena.grad[a:b]
        mine = g[self.rank * per:(self.rank + 1) * per]
        if self.nccl:
            out = torch.empty_like(mine)
            w = dist.reduce_scatter_tensor(out, g, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.pending.append((name, out, [w]))
        else:       # (gloo has no reduce-scatter: one reduce per destination rank; functional tests only)
            ws = [dist.reduce(g[r * per:(r + 1) * per], dst=dist.get_global_rank(self.group, r) if self.group is not None else r,
                              op=dist.ReduceOp.SUM, group=self.group, async_op=True) for r in range(self.world)]
            self.pending.append((name, mine, ws))

    def finish(self):
        """-> [(name, flat slice [lo, hi) of this rank, reduced gradient slice)]"""
        out = []
        for name, gshard, ws in self.pending:
            for w in ws:
                w.wait()
            a, b, per = self.spans[name]
            out.append((name, a + self.rank * per, a + (self.rank + 1) * per, gshard.clone() if not self.nccl else gshard))
        self.pending = []
        return out

    def all_gather_params(self, name):
        self.all_gather_span(self.arena.flat, name)

    def all_gather_span(self, flat, name):
        """every rank's slice of the table span of `flat` (the parameters, or an Adam moment of the same layout) to every rank"""
        a, b, per = self.spans[name]
        full = flat[a:b]
        mine = full[self.rank * per:(self.rank + 1) * per]
        dist.all_gather_into_tensor(full, mine if self.nccl else mine.clone(), group=self.group)


class LossScaler:
    """The policy of torch.cuda.amp.GradScaler (what accelerate wraps around the reference's fp16 training, zipnerf/train.py:44,215,331) as
    host state: the scale starts at `init_scale`, a step whose gradients hold a NaN / +-Inf is skipped and multiplies it by
    `backoff_factor`, `growth_interval` consecutive clean steps multiply it by `growth_factor`.  Same defaults as torch."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not (init_scale > 0 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and growth_interval >= 1):
            raise ValueError("LossScaler: init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self.scale, self.growth_factor, self.backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self.growth_interval, self.good_steps, self.skipped_steps = int(growth_interval), 0, 0

    def update(self, found_inf: bool) -> bool:
        """-> True when the optimizer step has to be skipped"""
        if found_inf:
            self.scale *= self.backoff_factor
            self.good_steps = 0
            self.skipped_steps += 1
            return True
        self.good_steps += 1
        if self.good_steps >= self.growth_interval:
            self.scale *= self.growth_factor
            self.good_steps = 0
        return False

    def state_dict(self):
        return dict(scale=self.scale, growth_factor=self.growth_factor, backoff_factor=self.backoff_factor, growth_interval=self.growth_interval,
                    good_steps=self.good_steps, skipped_steps=self.skipped_steps)

    def load_state_dict(self, d):
        self.scale, self.growth_factor, self.backoff_factor = float(d["scale"]), float(d["growth_factor"]), float(d["backoff_factor"])
        self.growth_interval, self.good_steps, self.skipped_steps = int(d["growth_interval"]), int(d["good_steps"]), int(d.get("skipped_steps", 0))


class ZipTrainer(_ArenaAdam):
    """Train step of the S-NeRF++ / zipnerf background model (s-nerfpp/zipnerf/train.py hot loop :218-331: Model.forward, the loss
    terms, loss.backward(), optimizer.step()) on the flat arenas: forward, ONE fused loss-tail launch (ops.zip_loss_tail: Charbonnier
    data term, disparity-L1 depth terms, semantic NLL, anti-interlevel and distortion regularisers, with their gradients), backward
    through the fused kernels, the RCCL all-reduce of the flat gradient arena (MLPs + the 3 hash tables, ~310 MB for waymo.gin) issued
    level by level so that it overlaps with the remaining backward, and one fused Adam launch with the 1/world mean folded in.  No device->host sync anywhere in the step: the loss terms stay on the
    device in `last_losses` (ops.ZIP_LOSS_NAMES order).

    `loss_cfg` overrides the reference defaults (internal/configs.py:60-66,85; train.py:253,272,298): charb_padding 0.001, data_mult
    1, depth_lambda 0.5, com_mult 0.2, sem_mult 0.04, pulse_width (0.03, 0.003), interlevel_mult 0.01, distortion_mult 0.005, mse False,
    hash_decay_mult 0.1 (`snerf_hash_decay`, one pass over the three tables, value appended to `last_losses`), d_smo_mult / s_smo_mult
    0.001 (train.py:281-282: the patch terms of `step(n_patch=...)`, `snerf_zip_smooth_loss`, values in `last_smooth_losses`).
    Further caller-defined terms on the ray histories go through `aux_loss_fn(ray_history) -> scalar` (torch autograd on detached
    leaf copies of every level's `weights`; its d(loss)/d(weights) is added to the fused tail's)."""

    def __init__(self, model, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, charb_padding=0.001, process_group=None, loss_cfg=None,
                 nonfinite="zero", grad_max_val=0.0, grad_max_norm=0.0, table_exchange="sharded", loss_scale=None, pose_net=None, pose_lr=1e-2,
                 pose_index="glo_idx"):
        """`pose_net` (a poses.LearnPoseV2; config.pose_refine, zipnerf/train.py:177-213, 338-344): the per-ray learned camera poses,
        trained by `step(pose="train")` and applied by `step(pose="apply")` on the device.  Its trained parameters move into a flat
        table with plain SGD (`self.pose`, a _PoseSGD; `pose_lr` = `self.pose.lr`, a plain attribute read at step time: assign the
        schedule's value, pn_lr_fn, before the step); `pose_index`: the batch key that holds each ray's table row (`cam_idx` stands in
        when the batch has no `glo_idx`).  loss_cfg `pose_depth_lambda` (0.0, train.py:256) replaces depth_lambda in a "train" step.
        `pose_state_dict()` / `load_pose_state_dict()`: the table's optimiser in torch.optim.SGD's layout.
        `loss_scale` (a number = static; default 4096 when the model computes in fp16, else 1): the gradients of the rendered outputs are
        multiplied by it before the backward -- so that the fp16 gradient buffers of the networks stay in fp16's normal range -- and the
        factor is undone inside the Adam launch (grad_scale), before clipping.  Overflowed (non-finite) gradients are dropped by
        `nonfinite` and counted in `dropped_nonfinite` (device int64: watch it in fp16 runs -- GradScaler would have skipped those steps).
        `loss_scale="dynamic"` (or a LossScaler): torch's GradScaler policy -- one pass over the gradient arena after the
        exchange (snerf_nonfinite_flag, + a 4-byte MAX all-reduce when the tables are sharded), ONE device->host read of the flag per
        step (as GradScaler.step does), a step with an overflow is skipped whole (parameters, m, v and the step count t untouched,
        gradients zeroed) and halves the scale; `scaler.skipped_steps` counts them.  The static scale keeps the step free of host syncs.
        `nonfinite`, `grad_max_val`, `grad_max_norm` = train_utils.clip_gradients (train_utils.py:234-243, run every step at
        zipnerf/train.py:336; configs.py:83-84 defaults 0 = off), folded into the Adam launch.  The reference always ends with
        param.grad.nan_to_num_(); "zero" (default) also drops +-Inf instead of mapping it to +-FLT_MAX (which would leave v = inf,
        i.e. that parameter frozen for good); "nan_to_num" reproduces the reference exactly."""
        self._arena_buffers(model, lr, betas, eps, nonfinite, grad_max_val, grad_max_norm, process_group)
        self.loss_cfg = dict(charb_padding=charb_padding)
        self.loss_cfg.update(loss_cfg or {})
        # hash-grid weight decay (train_utils.py:184-203; configs.py:74): a term on the parameters, not on the rays
        self.hash_decay_mult = float(self.loss_cfg.pop("hash_decay_mult", 0.1))
        # the patch terms (train.py:280-293; step(n_patch=...)): computed behind the fused tail, not arguments of it
        self.d_smo_mult, self.s_smo_mult = float(self.loss_cfg.pop("d_smo_mult", 0.001)), float(self.loss_cfg.pop("s_smo_mult", 0.001))
        self.last_smooth_losses, self._patch_own, self._patch_ws = None, {}, None
        self.pose_depth_lambda = float(self.loss_cfg.pop("pose_depth_lambda", 0.0))
        self.pose, self.pose_index, self.last_ray_grads = None, pose_index, None
        if pose_net is not None:
            self.pose = _PoseSGD(pose_net, model.arena.flat.device, pose_lr)
            self.side = (self.pose,)
        a = model.arena
        self.last_losses = None
        # running count of NaN / +-Inf gradient elements the Adam launches met (device int64, no host sync; read it when logging): a
        # persistently overflowing fp16 run with the static scale looks healthy otherwise -- the `nonfinite` policy drops them silently
        self.dropped_nonfinite = torch.zeros(1, dtype=torch.int64, device=a.flat.device)
        self.scaler = LossScaler() if isinstance(loss_scale, str) and loss_scale == "dynamic" else (loss_scale if isinstance(loss_scale, LossScaler) else None)
        if isinstance(loss_scale, str) and self.scaler is None:
            raise ValueError(f"loss_scale: a number, 'dynamic' or a LossScaler, not {loss_scale!r}")
        if self.scaler is not None:
            self.loss_scale = self.scaler.scale
            self._found_inf = torch.zeros(1, dtype=torch.int32, device=a.flat.device)
        else:
            self.loss_scale = float(loss_scale) if loss_scale is not None else (4096.0 if getattr(model, "dt", None) == ops.F16 else 1.0)
        # the hash tables' gradients: "sharded" (default for N > 1) = reduce-scatter + Adam on the rank's slice + all-gather of the updated
        # parameters (_TableShards); "allreduce" = part of the bucketed all-reduce like the MLP parameters (the reference's DDP behaviour)
        if table_exchange not in ("sharded", "allreduce"):
            raise ValueError(table_exchange)
        self.tables = [n + "encoder.embeddings" for n in model.names]
        self.shards = None
        if table_exchange == "sharded" and self.world > 1 and self.grad_max_norm <= 0 and \
                all((a.span(n)[1] - a.span(n)[0]) % self.world == 0 for n in self.tables):
            self.shards = _TableShards(a, self.tables, self.world, process_group)

    def _moments(self):
        """sharded table updates keep a rank's Adam moments current on its own slices only: a checkpoint gathers them (collective: every
        rank has to call state_dict())"""
        if self.shards is None:
            return self.m, self.v
        m, v = self.m.clone(), self.v.clone()
        for name in self.tables:
            self.shards.all_gather_span(m, name)
            self.shards.all_gather_span(v, name)
        return m, v

    def state_dict(self):
        sd = super().state_dict()
        if self.scaler is not None:
            sd["loss_scaler"] = self.scaler.state_dict()
        else:
            sd["static_loss_scale"] = float(self.loss_scale)
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)                    # (refuses before it writes: the scaler of a refused state stays as it was)
        if self.scaler is not None and "loss_scaler" in sd:
            self.scaler.load_state_dict(sd["loss_scaler"])
            self.loss_scale = self.scaler.scale
        elif self.scaler is None and "static_loss_scale" in sd and float(sd["static_loss_scale"]) != float(self.loss_scale):
            import warnings
            warnings.warn(f"resuming with a static loss scale of {self.loss_scale:g}; the checkpoint was trained with {float(sd['static_loss_scale']):g}")

    def _overflowed(self, a, shards):
        """dynamic loss scaling: the found-inf pass over the exchanged gradients and the scaler's update; -> True = the step is skipped
        (gradients zeroed; parameters, moments and t stay as they were)"""
        self._found_inf.zero_()
        ops.nonfinite_flag(a.grad, self._found_inf)
        if shards is not None:         # sharded tables: each rank sees the reduced gradient of its slices only -> agree on the flag
            for _, _, _, gshard in shards:
                ops.nonfinite_flag(gshard, self._found_inf)
            dist.all_reduce(self._found_inf, op=dist.ReduceOp.MAX, group=self.pg)
        if not self.scaler.update(bool(int(self._found_inf.item()))):
            return False
        a.grad.zero_()
        return True

    def _patch_targets(self, t, R, rows, dev):
        """the targets with the patch rows [0, rows) left out of the data, depth, depth-completion and semantic terms (train.py:231-264,
        296: mask_rgb): lossmult and the three masks with those rows zeroed, in buffers of the trainer -- the caller's tensors are not
        written.  The loss tail reads an absent lossmult, and an absent semantic_mask beside labels, as 1 on every row: those two become
        ones with zero patch rows; an absent depth_mask or complete_mask turns its term off and stays absent"""
        t = dict(t)
        for key in ("lossmult", "depth_mask", "complete_mask", "semantic_mask"):
            src = t.get(key)
            if src is None and not (key == "lossmult" or (key == "semantic_mask" and t.get("semantic") is not None)):
                continue
            own = self._patch_own.get(key)
            if own is None or own.shape[0] != R:
                own = self._patch_own[key] = torch.empty(R, dtype=torch.float32, device=dev)
            if src is None:
                own.fill_(1.0)
            else:
                own.copy_(src.reshape(R))
            own[:rows].zero_()
            t[key] = own
        return t

    def _patch_terms(self, fin, target_rgb, n_patch, p, patch_mask, G, ls, dev):
        """d_smo + s_smo of the patch rows (ops.zip_smooth_loss) ADDED into the tail's g_depth / g_sem (zero buffers where the tail had
        none), the loss scale in their gradients -> the sum of the two values (device scalar); `last_smooth_losses` = {d_smo, s_smo}"""
        rows, R = n_patch * p * p, target_rgb.shape[0]
        sem = fin.get("semantic")
        if G["depth"] is None:
            G["depth"] = torch.zeros(R, dtype=torch.float32, device=dev)
        if sem is not None and G["semantic"] is None:
            G["semantic"] = torch.zeros(R, sem.shape[1], dtype=torch.float32, device=dev)
        n_ws = ops.zip_smooth_loss_ws(n_patch)
        if self._patch_ws is None or self._patch_ws.numel() < n_ws:
            self._patch_ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
        out = torch.zeros(4, dtype=torch.float32, device=dev)
        ops.zip_smooth_loss(target_rgb[:rows], fin["depth"].reshape(-1)[:rows], None if sem is None else sem[:rows], patch_mask, n_patch, p,
                            d_mult=self.d_smo_mult, s_mult=self.s_smo_mult, grad_mult=ls, out=out, g_depth=G["depth"].reshape(-1)[:rows],
                            g_sem=None if sem is None else G["semantic"][:rows], accumulate=True, ws=self._patch_ws)
        self.last_smooth_losses = out[:2]
        return out[0] + out[1]

    def step(self, batch, target_rgb, train_frac=1.0, rand=True, aux_loss_fn=None, draws=None, sample_n=7, sample_m=3, targets=None, zero_glo=False,
             n_patch=None, patch_size=None, patch_mask=None, pose=None, ray_grads=False):
        """`pose` (with a `pose_net`): "train" = a step of the refinement window (train.py:180-197, 256, 340-344) -- the rays are moved by
        the rows of their cameras (ops.pose_table, ops.pose_rays_apply), the loss tail runs with depth_lambda = `pose_depth_lambda` (0:
        `depth` and `d_complete` vanish), the backward also returns the ray gradients, ops.pose_rays_grad reduces them camera by camera
        and the table takes its SGD step after the model's update (skipped with it when a dynamic loss scale overflows); "apply" = a step
        after the window or with a loaded table (train.py:201-213): the rays are moved, the rest is the plain step, the table is not
        touched.  `ray_grads=True` leaves d loss / d (origins, directions, viewdirs, base_x, base_y) of the rays the model saw in
        `last_ray_grads` (the loss scale divided out): for callers who keep a pose optimiser of their own (zipnerf.apply_pose).
        `targets` (all optional, per ray): lossmult [R] (the reference's mask_rgb as 0/1 floats), depth [R] + depth_mask [R]
        (+ complete_mask [R]), semantic int32 labels [R] + semantic_mask [R].  `zero_glo` (models with GLO vectors): train with zero
        vectors instead of the rows batch['cam_idx'] selects (zipnerf/train.py:235 passes zero_glo=False).
        `n_patch` > 0 with `patch_size` = p (a batch of zipnerf.PatchRayBatcher: n_patch = its n_patch_local): rows [0, n_patch p^2) are
        whole p x p patches.  They leave the data, depth, depth-completion and semantic terms (train.py:231-264, 296) and carry the patch
        terms of train.py:280-293 instead, d_smo and s_smo (loss_cfg d_smo_mult / s_smo_mult, 0.001 each; s_smo only with a semantic
        head), computed behind the loss tail by ops.zip_smooth_loss on target_rgb and the NeRF level's depth and semantic outputs;
        interlevel and distortion keep every ray.  `patch_mask` [n_patch p^2]: the batch's mask on those rows, > 0 = masked out (None =
        all valid, the reference's use_mask = False).  The two values are in `last_smooth_losses` (device; None after a step without
        patches) and in the returned loss; `last_losses` is what it is without patches.  With several ranks each averages over its own
        patches; a rank that has none passes n_patch = 0 (an empty patch_mask is accepted there) and takes the plain step."""
        m = self.model
        m._zero_glo = bool(zero_glo)
        dev = m.arena.flat.device
        R = batch['origins'].shape[0]
        cam = self._pose_index(batch, pose, R, dev)
        n_patch, p, t = self._step_args(R, target_rgb, targets or {}, n_patch, patch_size, patch_mask, dev)
        train = pose == "train"
        if pose is not None:
            batch, unmoved = self._pose_move(batch, cam, dev)
        if draws is None:
            draws = m._draws(R, rand, dev, sample_n)
        levels, ctx = m._run(batch, True, float(train_frac), draws, sample_n, sample_m)
        loss, G, g_w = self._loss_and_grads(levels, target_rgb, t, n_patch, p, patch_mask, aux_loss_fn, dev,
                                            depth_lambda=self.pose_depth_lambda if train else None)
        mine, rg = self._backward(ctx, G, g_w, ray_grads=ray_grads or train)
        if train:
            ps = self.pose
            ops.pose_rays_grad(ps.net.r.data, ps.net.t_ratio, cam, *rg, *unmoved[1:], ps.g.get("r"), ps.g.get("t"), ws=ps.workspace(R))
        ls = self.loss_scale
        self.last_ray_grads = ([g if ls == 1.0 else g * (1.0 / ls) for g in rg] if ray_grads else None)
        if self._update(mine):
            if train:
                self.pose.train(self.world, self.pg, self.nonfinite, loss_scale=ls, grad_max_val=self.grad_max_val,
                                grad_max_norm=self.grad_max_norm, dropped=self.dropped_nonfinite)
        elif train:
            self.pose.grad.zero_()
        return loss, levels

    def _pose_index(self, batch, pose, R, dev):
        """checks of step's `pose` argument, before any launch -> the rays' table rows as fp32 [R] on the device (None without `pose`)"""
        if pose is None:
            return None
        if pose not in ("train", "apply"):
            raise ValueError(f"pose: None, 'train' or 'apply', not {pose!r}")
        if self.pose is None:
            raise ValueError(f"step(pose={pose!r}) needs a ZipTrainer built with pose_net=")
        key = self.pose_index if self.pose_index in batch else "cam_idx"
        if key not in batch:
            raise ValueError(f"step(pose={pose!r}): the batch has neither {self.pose_index!r} nor 'cam_idx' (each ray's row of the pose table)")
        if batch[key].numel() != R:
            raise ValueError(f"batch[{key!r}]: one table row per ray ({R}), got {batch[key].numel()} values")
        self.pose.check_views()
        return batch[key].detach().to(dev, torch.float32).reshape(R).contiguous()

    def _pose_move(self, batch, cam, dev):
        """-> (a new batch with every ray moved by the table row of its camera, the five unmoved ray tensors as the kernels read them)"""
        from .zipnerf import POSE_RAY_KEYS
        net = self.pose.net
        unmoved = [batch[k].detach().to(dev, torch.float32).reshape(-1, 3).contiguous() for k in POSE_RAY_KEYS]
        table = ops.pose_table(net.r.data, net.t.data, net.t_ratio)
        batch = dict(batch)
        batch.update(zip(POSE_RAY_KEYS, ops.pose_rays_apply(table, cam, *unmoved)))
        return batch, unmoved

    def pose_state_dict(self):
        """the pose optimiser's state in torch.optim.SGD's layout (the table itself is `pose_net.state_dict()`)"""
        return self.pose.state_dict()

    def load_pose_state_dict(self, sd):
        self.pose.load_state_dict(sd)

    def _step_args(self, R, target_rgb, t, n_patch, patch_size, patch_mask, dev):
        """checks of step's patch arguments -> (n_patch, p, the targets the loss tail sees)"""
        n_patch = int(n_patch or 0)
        if n_patch < 0 or (n_patch > 0 and patch_size is None):
            raise ValueError("n_patch: a count of patches >= 0, with patch_size")
        if n_patch == 0:
            self.last_smooth_losses = None             # (a step without patches, a rank with none: nothing stale for a logger)
            if patch_mask is not None and patch_mask.numel() != 0:    # (the empty mask of a rank without patches is a plain step)
                raise ValueError("patch_mask without n_patch")
            return 0, None, t
        p = int(patch_size)
        if not 2 <= p <= 32:
            raise ValueError(f"patch_size {p}: 2..32")
        if n_patch * p * p > R:
            raise ValueError(f"{n_patch} patches of {p} x {p} rays are more than the batch's {R} rows")
        if patch_mask is not None and patch_mask.numel() != n_patch * p * p:
            raise ValueError(f"patch_mask: one value per patch row ({n_patch * p * p}), got {patch_mask.numel()}")
        if target_rgb.shape[0] != R:
            raise ValueError("target_rgb: one row per ray")
        return n_patch, p, self._patch_targets(t, R, n_patch * p * p, dev)

    def _loss_and_grads(self, levels, target_rgb, t, n_patch, p, patch_mask, aux_loss_fn, dev, depth_lambda=None):
        """the fused loss tail, hash decay, the patch terms and `aux_loss_fn` -> (loss, the tail's output gradients G with the loss scale
        in them, the three levels' weight gradients).  `depth_lambda`: this step's value in place of loss_cfg's (a pose-training step)"""
        m = self.model
        fin = levels[2]
        cfg = self.loss_cfg if depth_lambda is None else dict(self.loss_cfg, depth_lambda=depth_lambda)
        with_depth = t.get("depth") is not None
        with_sem = t.get("semantic") is not None and fin.get("semantic") is not None
        out, G = ops.zip_loss_tail(fin["rgb"], target_rgb, t.get("lossmult"), depth=fin["depth"] if with_depth else None,
                                   tdepth=t.get("depth"), dmask=t.get("depth_mask"), cmask=t.get("complete_mask"),
                                   sem=fin["semantic"] if with_sem else None, labels=t.get("semantic") if with_sem else None,
                                   smask=t.get("semantic_mask"), hist=[(levels[l]["sdist"], levels[l]["weights"]) for l in range(3)],
                                   **cfg)
        decay = torch.zeros(1, dtype=torch.float32, device=dev)
        if self.scaler is not None:
            self.loss_scale = self.scaler.scale
        ls = self.loss_scale
        if ls != 1.0:
            for g in G.values():
                if g is not None:
                    g.mul_(ls)
        if self.hash_decay_mult > 0:
            for lvl, pre in enumerate(m.names):            # identical on every rank: the all-reduced mean leaves it unchanged
                e = m.encs[lvl]
                ops.hash_decay(m.arena.p[pre + "encoder.embeddings"], m.arena.g[pre + "encoder.embeddings"], m.dev_offsets[lvl], e.L, e.C,
                               self.hash_decay_mult, decay, grad_mult=ls)
        self.last_losses = torch.cat([out[4:], decay])     # ops.ZIP_LOSS_NAMES + ("hash_decay",)
        loss = out[4] + out[6:].sum() + decay[0]
        if n_patch > 0:
            pm = None if patch_mask is None else patch_mask.detach().reshape(-1).to(dev, torch.float32).contiguous()
            loss = loss + self._patch_terms(fin, target_rgb, n_patch, p, pm, G, ls, dev)
        g_w = [G["w0"], G["w1"], G["w2"]]
        if aux_loss_fn is not None:
            with torch.enable_grad():
                leaves = [levels[l]["weights"].detach().requires_grad_(True) for l in range(3)]
                hist = [dict(sdist=levels[l]["sdist"].detach(), tdist=levels[l]["tdist"].detach(), weights=leaves[l]) for l in range(3)]
                aux = aux_loss_fn(hist)
                gs = torch.autograd.grad(aux, leaves, allow_unused=True)
            gs = [b if (b is None or ls == 1.0) else b * ls for b in gs]
            g_w = [a if b is None else (b if a is None else a + b) for a, b in zip(g_w, gs)]
            loss = loss + aux.detach()
        return loss, G, g_w

    def _backward(self, ctx, G, g_w, ray_grads=False):
        """the backward pass with the gradient exchange under it -> (this rank's reduced table slices (_TableShards.finish), or None;
        with `ray_grads` d loss / d (origins, directions, viewdirs, base_x, base_y), the loss scale in them, else None)"""
        m = self.model
        ex = _GradExchange(m.arena, self.world, self.pg)
        sh = self.shards
        if sh is not None:
            for n in self.tables:                      # the table spans do not ride in the all-reduce buckets
                ex.done.append(m.arena.span(n))

        def level_done(prefix):
            # a level's gradients are final: its table starts its reduce-scatter, its MLP parameters their all-reduce -- the NeRF level
            # (240 MB of table gradient) is on the wire while the two proposal levels' backward runs
            if sh is not None and isinstance(prefix, str) and prefix + "encoder.embeddings" in sh.spans:
                sh.reduce_scatter(prefix + "encoder.embeddings")
            ex(prefix)
        rg = m._backward(ctx, [(None, None, None, g_w[0]), (None, None, None, g_w[1]), (G["rgb"], G["depth"], None, g_w[2], G["semantic"])],
                         on_done=level_done, ray_grads=ray_grads)
        ex.finish()
        return (sh.finish() if sh is not None else None), rg

    def _update(self, mine):
        """the overflow test of a dynamic loss scale, then Adam with the loss scale and the data-parallel mean folded in: one launch over the
        arena, or with sharded tables (`mine`) one per table slice of this rank and one per stretch between the table spans
        -> False when the step was skipped for an overflow"""
        a, sh = self.model.arena, self.shards
        if self.scaler is not None and self._overflowed(a, mine):
            return False
        self.t += 1
        grad_scale = 1.0 / (self.world * self.loss_scale)
        if sh is None:
            self._arena_adam(grad_scale, dropped=self.dropped_nonfinite)
            return True
        # tables: this rank's slice only, then the updated slices are gathered; everything between the table spans: the usual pass
        hygiene = dict(grad_max_val=self.grad_max_val, dropped=self.dropped_nonfinite)
        for name, lo, hi, gshard in mine:
            self.adam(grad_scale, self.nonfinite, lo, hi, gshard, **hygiene)
        pos = 0
        for ta, tb in sorted(a.span(n) for n in self.tables) + [(a.numel, a.numel)]:
            if ta > pos:
                self.adam(grad_scale, self.nonfinite, pos, ta, **hygiene)
            if tb > ta:
                a.grad[ta:tb].zero_()
            pos = max(pos, tb)
        for name in self.tables:
            sh.all_gather_params(name)
        a.bump()
        return True


class _NetAdam(_AdamState):
    """_AdamState over the arena of ONE network of a ClassicTrainer: its fused Adam launch, its device step / lr words and its part of
    the warm-up snapshot.  The moments are the network's slices of the trainer's moment buffers; step count and hyper-parameters are
    the trainer's (one optimiser over both networks, like torch.optim.Adam(grad_vars))."""
    what = "network"
    lr, betas, eps = (property(lambda self, k=k: getattr(self.owner, k)) for k in ("lr", "betas", "eps"))
    t = property(lambda self: self.owner.t, lambda self, v: setattr(self.owner, "t", v))

    def __init__(self, owner, net, m, v):
        self.owner, self.net, self.m, self.v = owner, net, m, v

    def _buffers(self):
        return self.net.arena.flat, self.net.arena.grad


class ClassicTrainer(_CapturedStep, _AdamState):
    """Train step of the classic render_rays path (path B; the stock loop around s-nerf/model/render.py:281-409: render_rays,
    img2mse on the fine and the coarse colour map, loss.backward(), optimizer.step()) without the autograd round trip: the operators
    of classic.render_rays called directly, ONE loss-tail pair of launches (ops.classic_loss_tail: loss, psnr and d loss / d rgb), the
    compositing and network backward passes into the flat gradient arenas, the all-reduce of each arena, and one fused Adam launch per
    arena with the 1 / world mean (and the loss scale) folded in.  No autograd graph, no per-parameter gradient clones, no host read.

    Arguments as render_rays' (`ClassicTrainer(**render_kwargs_train)` works: create_nerf's `use_viewdirs` / `ndc` entries belong to
    render() and are accepted and ignored; `network_query_fn` is kept for that signature only: the networks embed inside their first
    kernel).  `network_fine=None` with N_importance > 0 runs both passes through `network_fn`, whose arena then collects both passes'
    gradients; N_importance = 0 is the one-level render.  NeRF_RGB networks (a frozen alpha model) and `ert` are not offered.
    `lr` is a plain attribute read at step time: assign the schedule's value (classic.lrate_decay) before a step or a replay.
    `nonfinite`: ops.adam_step's policy.  `loss_scale`: the tail's gradients are multiplied by it before the backward passes and the
    factor is undone inside the Adam launches.
    `state_dict()` / `load_state_dict()`: torch.optim.Adam's layout over create_nerf's grad_vars order -- the coarse network's
    parameters, then the fine one's -- with one step count: the `optimizer_state_dict` of the reference's checkpoints
    (render.py:165-278; classic.create_nerf)."""
    what, named = "classic", True

    def __init__(self, network_fn, network_query_fn=None, N_samples=64, N_importance=0, network_fine=None, lr=5e-4, betas=(0.9, 0.999), eps=1e-8,
                 perturb=1., lindisp=False, white_bkgd=False, raw_noise_std=0., nonfinite="zero", loss_scale=1.0, process_group=None,
                 exchange_when_single=False, use_viewdirs=None, ndc=None):
        from . import classic
        nets = [network_fn] + ([network_fine] if network_fine is not None else [])
        for net in nets:
            if not isinstance(net, classic.NeRF):
                raise ValueError("ClassicTrainer: network_fn / network_fine must be snerf_amd.classic.NeRF modules (network_fn is needed: the "
                                 "no_coarse route belongs to NeRF_RGB)")
            if not net._alpha_head:
                raise ValueError("ClassicTrainer: NeRF_RGB (the colour network over a frozen alpha model) is not offered")
        if network_fine is not None and int(N_importance) <= 0:
            raise ValueError("ClassicTrainer: network_fine is evaluated on the importance samples only: it needs N_importance > 0")
        if network_fine is network_fn:
            raise ValueError("ClassicTrainer: pass network_fine=None to run both passes through network_fn")
        if network_fine is not None and network_fine.arena.flat.device != network_fn.arena.flat.device:
            raise ValueError("ClassicTrainer: both networks on one device")
        if int(N_samples) < 2 or int(N_importance) < 0 or not float(loss_scale) > 0:
            raise ValueError("ClassicTrainer: N_samples >= 2, N_importance >= 0, loss_scale > 0")
        self.network_fn, self.network_fine, self.network_query_fn = network_fn, network_fine, network_query_fn
        self.N_samples, self.N_importance = int(N_samples), int(N_importance)
        self.lr, self.betas, self.eps, self.t = lr, tuple(betas), eps, 0
        self.perturb, self.lindisp, self.white_bkgd, self.raw_noise_std = float(perturb), bool(lindisp), bool(white_bkgd), float(raw_noise_std)
        self.nonfinite, self.loss_scale = nonfinite, float(loss_scale)
        self.pg = process_group
        live = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if live else 1
        self.single_rank_exchange = bool(exchange_when_single) and live
        dev = network_fn.arena.flat.device
        sizes = [net.arena.numel for net in nets]
        self.m, self.v = torch.zeros(sum(sizes), dtype=torch.float32, device=dev), torch.zeros(sum(sizes), dtype=torch.float32, device=dev)
        self._base = [0]
        for k in sizes:
            self._base.append(self._base[-1] + k)
        self.nets = [_NetAdam(self, net, self.m[a:a + k], self.v[a:a + k]) for net, a, k in zip(nets, self._base, sizes)]
        for net in nets:
            net.arena.grad.zero_()
        self._const, self._ws = {}, None

    # ---- the optimiser state ------------------------------------------------------------------------------------------------------
    def _layout(self):
        """create_nerf's grad_vars order: list(model.parameters()) + list(model_fine.parameters()), offsets into the moment buffers"""
        out = []
        for tag, x, base in zip(("network_fn.", "network_fine."), self.nets, self._base):
            a = x.net.arena
            out += [(tag + n, base + a._offs[n][0], a._offs[n][1], a.shapes[n]) for n, _ in x.net.named_parameters()]
        return out

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        for x in self.nets:
            if x.step_dev is not None:
                x.step_dev.fill_(self.t)

    def broadcast_parameters(self, src=0):
        if self.world > 1:
            for x in self.nets:
                dist.broadcast(x.net.arena.flat, src=src, group=self.pg)
                x.net.arena.bump()

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def _constant(self, key, make):
        """a device constant built once (render_rays uploads its linspace every call)"""
        hit = self._const.get(key)
        if hit is None:
            hit = self._const[key] = make()
        return hit

    def _network(self, net, pts, viewdirs, S):
        """run_network's preparation of (inputs, viewdirs) and the network's training forward -> (raw [n S, C], saved)"""
        if net.use_viewdirs != (viewdirs is not None):       # (as run_network)
            raise TypeError("ClassicTrainer: ray rows with view directions ([N, 11]) go with networks built with use_viewdirs=True, and only "
                            "with them")
        net._check_arena()
        vd = None
        if net.use_viewdirs:
            vd = viewdirs if viewdirs.stride(-1) == 1 else viewdirs.contiguous()
        return net.net.forward(pts.reshape(-1, 3), vd, S, True)

    def _forward_backward(self, ray_batch, target_rgb, t_rand=None, u=None, noise=None, on_done=None):
        """draws, both passes forward, the loss tail, both passes backward into the gradient arenas (no exchange, no optimiser).
        `on_done(i)`: network i's gradients are final"""
        from . import classic
        S, Ni = self.N_samples, self.N_importance
        coarse = self.network_fn
        fine = self.network_fine if self.network_fine is not None else coarse
        if ray_batch.dim() != 2 or ray_batch.shape[0] == 0 or ray_batch.shape[1] not in (8, 11):
            raise ValueError("ClassicTrainer: ray_batch is render_rays' [N, 8 | 11] = [o3, d3, near, far, (viewdir3)] with N >= 1")
        dev = coarse.arena.flat.device
        rb = ray_batch.detach().to(dev, torch.float32)
        if rb.stride(-1) != 1:
            rb = rb.contiguous()
        N = rb.shape[0]
        tgt = target_rgb.detach().to(dev, torch.float32).contiguous()
        if tuple(tgt.shape) != (N, 3):
            raise ValueError("ClassicTrainer: target_rgb is [N, 3]")
        rays_d = rb[:, 3:6]
        viewdirs = rb[:, -3:] if rb.shape[-1] > 9 else None
        base = self._constant(("base", S), lambda: torch.linspace(0., 1., steps=S).to(dev))
        if self.perturb > 0. and t_rand is None:
            t_rand = torch.rand(N, S, device=dev)
        z_vals = ops.stratified(base, None if t_rand is None else t_rand.contiguous().float(), rb[:, 6], rb[:, 7], N, 0, self.lindisp)
        noises = list(noise) if isinstance(noise, (tuple, list)) else [noise, None]
        std = self.raw_noise_std

        def level(net, z, given):
            """one pass: points, network, compositing -> (raw, saved, noise, (rgb, disp, acc, weights, depth))"""
            raw, saved = self._network(net, ops.classic_points(rb, z), viewdirs, z.shape[1])
            if given is None and std > 0.:             # raw2outputs' draw (run_nerf_helpers.py:399-401)
                given = torch.randn(N, z.shape[1], device=dev) * std
            if given is not None:
                given = given.to(dev, torch.float32).contiguous()
            return raw, saved, given, ops.classic_composite_fwd(raw, given, z, rays_d, self.white_bkgd)
        raw0, saved0, noise0, (rgb0, disp0, acc0, w0, depth0) = level(coarse, z_vals, noises[0])
        ret = {"rgb_map": rgb0, "disp_map": disp0, "acc_map": acc0, "depth_map": depth0, "z_vals_map": z_vals, "weights": w0}
        if Ni > 0:
            if u is None and self.perturb == 0.:
                u = self._constant(("u", Ni), lambda: torch.linspace(0., 1., steps=Ni).to(dev))
            u = classic._draw_u(N, Ni, False, False, u, dev)
            z_samples, _, z_std = ops.classic_sample_pdf(z_vals, w0, u, True, False, True)      # (no gradient: render.py:381 detaches)
            z_all = ops.classic_merge_sort(z_vals, z_samples)
            raw1, saved1, noise1, (rgb1, disp1, acc1, w1, depth1) = level(fine, z_all, noises[1])
            ret.update(rgb_map=rgb1, disp_map=disp1, acc_map=acc1, depth_map=depth1, rgb0=rgb0, disp0=disp0, acc0=acc0, z_std=z_std)
        # ---- the loss tail: loss, psnr and the gradients of both colour maps
        need = ops.classic_loss_tail_ws(N)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        if Ni > 0:
            out, g_rgb, g_rgb0 = ops.classic_loss_tail(rgb1, rgb0, tgt, ws=self._ws)
        else:                                            # (the one-level render: its only colour map is the coarse pass's)
            out, g_rgb0, g_rgb = ops.classic_loss_tail(rgb0, None, tgt, ws=self._ws)
        if self.loss_scale != 1.0:
            for g in (g_rgb, g_rgb0):
                if g is not None:
                    g.mul_(self.loss_scale)
        self.last_grads = (g_rgb, g_rgb0)
        ret["losses"] = out                              # {loss, img_loss, img_loss0, psnr}: stays on the device
        # ---- backward: the fine pass, then the coarse one (autograd's order), each from its colour map's gradient alone

        def level_bwd(net, raw, saved, nz, z, maps, g):
            _, _, acc, w, depth = maps
            d_raw = torch.zeros_like(raw)
            ops.classic_composite_bwd(raw, nz, z, rays_d, self.white_bkgd, w, acc, depth, g, None, None, None, None, d_raw)
            net.net.backward(d_raw, saved)
        if Ni > 0:
            level_bwd(fine, raw1, saved1, noise1, z_all, (rgb1, disp1, acc1, w1, depth1), g_rgb)
            if on_done is not None and fine is not coarse:
                on_done(1)
        level_bwd(coarse, raw0, saved0, noise0, z_vals, (rgb0, disp0, acc0, w0, depth0), g_rgb0)
        if on_done is not None:
            on_done(0)
        return out[0], ret

    def loss_and_grads(self, ray_batch, target_rgb, t_rand=None, u=None, noise=None):
        """forward, loss tail and backward: the gradients of the LOCAL mean are ADDED into every network's `arena.grad` (times
        `loss_scale`); no exchange, no Adam.  -> (loss, out) as `step`"""
        return self._forward_backward(ray_batch, target_rgb, t_rand, u, noise)

    def _exchanges(self):
        return [_GradExchange(x.net.arena, self.world, self.pg, self.single_rank_exchange) for x in self.nets]

    def _update(self):
        """one fused Adam launch per arena: folds the data-parallel mean, the loss scale, the non-finite policy and zero_grad"""
        self.t += 1
        scale = 1.0 / (self.world * self.loss_scale)
        for x in self.nets:
            x.adam(scale, self.nonfinite)
            x.net.arena.bump()

    def step(self, ray_batch, target_rgb, t_rand=None, u=None, noise=None):
        """One training step on `ray_batch` [N, 8 | 11] (render_rays' rows; a classic.RayBatcher's) and `target_rgb` [N, 3]; neither is
        written.  `t_rand` [N, N_samples] / `u` [N, N_importance] replace the torch.rand draws of render_rays; `noise` (one tensor
        [N, N_samples], or a pair with the fine pass's [N, N_samples + N_importance]) replaces raw2outputs' randn * raw_noise_std and is
        used as it is.  -> (loss, out): the loss as a device scalar, out = render_rays' maps (rgb_map, disp_map, acc_map, depth_map,
        z_vals_map, weights, and with N_importance > 0 rgb0, disp0, acc0, z_std) plus `losses` = the device vector
        {loss, img_loss, img_loss0, psnr}.  world > 1: every rank steps on its own shard and forms its own mean; the arenas' gradients are
        summed over the ranks (the fine network's under the coarse backward pass) and Adam takes 1 / world of the sum."""
        ex = self._exchanges()
        loss, out = self._forward_backward(ray_batch, target_rgb, t_rand, u, noise, on_done=lambda i: ex[i](""))
        for e in ex:
            e.finish()
        self._update()
        return loss, out

    # ---- hipGraph capture of the whole step --------------------------------------------------------------------------------------
    def capture(self, ray_batch=None, target_rgb=None, warmup=3, batcher=None):
        """Capture one full step (the torch RNG draws, forward, loss tail, backward, and for world 1 the Adam launches, with step count
        and learning rate in device memory) in a hipGraph on one stream; `replay()` then runs a step with one graph launch.  Without a
        batcher the graph reads the GIVEN tensors: refresh the batch by copying into them.  `batcher` (classic.RayBatcher): its draw
        (`next_into`, one launch) is the first node, every replay trains on a fresh batch -- the k-th on the batch an eager batcher
        draws at step s0 + k -- and `self.batch` = (ray_batch, target_rgb) are its buffers.  The `warmup` steps are real steps on the
        capture batch: parameters, moments, step count and the batcher's counter are snapshotted before and restored after them
        (the torch RNG does advance).  world > 1 (every rank calls capture / replay together): the graph ends with the backward, and
        `replay()` follows it with the all-reduces and the Adam launches."""
        if batcher is None and (ray_batch is None or target_rgb is None):
            raise ValueError("ClassicTrainer.capture: give ray_batch= and target_rgb=, or batcher=")
        buf = None
        if batcher is not None:
            buf = batcher.buffers()
            ray_batch, target_rgb = buf["rays"], buf["rgb"]
        self.batch = (ray_batch, target_rgb)
        return self._capture(warmup, batcher, buf, lambda: self.step(ray_batch, target_rgb), lambda: self._forward_backward(ray_batch, target_rgb))

    def _trained(self):
        return self.nets

    def _counted(self):
        return [self]                                    # (the nets' `t` is the trainer's: one count for both)

    def _bump_restored(self):
        for x in self.nets:
            x.net.arena.bump()

    def _after_graph(self):
        for e in self._exchanges():
            e.finish()                                   # one all-reduce per gradient arena
        self._update()
