"""Learned depth confidence (depth_conf = True, precompute_conf = True of both shipped S-NeRF configs): the per-image mixing weights of
s-nerf/model/confidence.py:65-73 over precomputed per-pixel confidence maps, as calc_final_confidence (:187-206) mixes them:

    conf = sum_k sigmoid(lambdas[k, img]) map_k / sum_k sigmoid(lambdas[k, img]),        conf = 1 on sky pixels (skymask = True)

`Confidence` keeps the reference's parameter name (`lambdas`), so the `confidence` entry of a reference checkpoint loads with
`load_state_dict`; `ConfidenceMaps` holds what `precompute_conf_map` returned on the device.  Training on the device goes through
`MipTrainer(conf_net=, conf_maps=)`: the table column is mixed for the batch by `snerf_conf_apply`, the loss tail returns
d loss / d conf, and `snerf_conf_grad` reduces it to the column's gradient; `conf_grad_chain` below is that kernel's host model in
float64.  `calc_final_confidence` is the same pair of kernels under autograd, for callers who keep their own loop.

The maps themselves come from `precompute_conf_map` below (also a method of `Confidence`, with the reference's signature): the rgb,
ssim and depth modes of get_reproj_conf (model/loss.py:271-327) -- reprojection with a bilinear gather, 11 x 11 Gaussian SSIM, two
global reductions per (base image, neighbour) pass -- computed by `snerf_reproj_conf` on the tensors an `ImageRayBatcher` already keeps
on the device; `ConfidenceMaps` gathers device maps on their device, so precompute -> ConfidenceMaps -> MipTrainer never leaves
the GPU.  The SSIM constants are those of L = 1: the images are floats in [0, 1], or uint8 decoded as float32(k / 255.0) like
the batcher does (the reference picks L from the data: 255 when max(img) > 128).

Not covered: the `vgg` mode (it needs torchvision's pretrained VGG-19; a VGG map computed elsewhere can be added to the dicts, since
ConfidenceMaps takes any mode names), the flow branch (unfinished in the reference: it stops in pdb.set_trace()), precompute_conf =
False (the maps recomputed every step from the learned poses: needs d maps / d pose), and Path C."""
import numpy as np
import torch
import torch.nn as nn

from . import ops

MAX_MODES = 8


class Confidence(nn.Module):
    def __init__(self, modes, images_num, tau=0.2):
        """`modes`: the names of the confidence maps that are mixed, in mixing order; `lambdas` [len(modes), images_num] starts at
        zero: every mode weighs the same.  `tau` (the temperature the maps were computed with) is kept for the caller."""
        super().__init__()
        self.modes = list(modes)
        if not 1 <= len(self.modes) <= MAX_MODES:
            raise ValueError(f"Confidence: 1..{MAX_MODES} modes, got {len(self.modes)}")
        self.images_num = int(images_num)
        self.lambdas = nn.Parameter(torch.zeros((len(self.modes), self.images_num), dtype=torch.float32), requires_grad=True)
        self.tau = tau

    def precompute_conf_map(self, args, cam_index, images, depth_gts, poses, intrinsics, i_train, flow=None, batcher=None, device=None):
        """confidence.py:78-85 on the device, for this model's modes and tau -> a list with one {mode: [H*W] fp32 device tensor} per
        position of i_train; `flow` is accepted only as None (see `precompute_conf_map` below)"""
        if flow is not None:
            raise NotImplementedError(_NO_FLOW)
        return precompute_conf_map(args, cam_index, images, depth_gts, poses, intrinsics, i_train, modes=self.modes, tau=self.tau,
                                   batcher=batcher, device=device)

    def load_state_dict(self, state_dict, *args, **kwargs):
        """the `confidence` entry of a reference checkpoint: its frozen VGG feature network (`vgg_loss.*`, vgg_loss = True) only serves
        the computation of the maps and is dropped"""
        kept = {k: v for k, v in state_dict.items() if not k.startswith("vgg_loss.")}
        return super().load_state_dict(kept, *args, **kwargs)


def build_confidence_model(args, N, device):
    """confidence.py:171-185: the mode list of the arguments and the table's own Adam (lr 1e-3) -> (Conf, optimizer_conf)"""
    mode = []
    if not args.no_reproj:
        mode += ["rgb", "ssim"]
    if not args.no_geometry:
        mode += ["depth"]
    if args.vgg_loss:
        mode += ["vgg"]
    conf = Confidence(mode, images_num=N, tau=args.tau).to(device)
    optimizer_conf = torch.optim.Adam([{"params": [p for p in conf.parameters() if p.requires_grad], "lr": 1e-3}])
    return conf, optimizer_conf


_NO_FLOW = ("the flow branch of the confidence maps is unfinished in the reference (reproj_flow_err stops in pdb.set_trace()) and is not "
            "computed here; a map computed elsewhere can still be added to the dicts: ConfidenceMaps takes any mode names")
_NO_VGG = ("the 'vgg' confidence map needs torchvision's pretrained VGG-19 and is not computed here; a VGG map computed elsewhere can still "
           "be added to the dicts precompute_conf_map returns: ConfidenceMaps takes any mode names")


def select_conf_neighbours(i_train, cam_index, p, conf_num):
    """sel_ids of select_conf_depends (confidence.py:125-135) for the image at position p of i_train: for k = 1..conf_num first
    i_train[p + k], then i_train[p - k], each only when the position exists and the image shares the base's camera.  The order matters:
    the last neighbour's depth mask zeroes the maps."""
    it = [int(i) for i in np.asarray(i_train.cpu() if torch.is_tensor(i_train) else i_train).reshape(-1)]
    cam = np.asarray(cam_index.cpu() if torch.is_tensor(cam_index) else cam_index).reshape(-1)
    p = int(p)
    sel = []
    for k in range(1, int(conf_num) + 1):
        if p + k < len(it) and cam[it[p]] == cam[it[p + k]]:
            sel.append(it[p + k])
        if p - k >= 0 and cam[it[p]] == cam[it[p - k]]:
            sel.append(it[p - k])
    return sel


def _modes_of(args):
    """build_confidence_model's mode list (confidence.py:171-178)"""
    mode = []
    if not getattr(args, "no_reproj", False):
        mode += ["rgb", "ssim"]
    if not getattr(args, "no_geometry", False):
        mode += ["depth"]
    if getattr(args, "vgg_loss", False):
        mode += ["vgg"]
    return mode


def precompute_conf_map(args, cam_index, images, depth_gts, poses, intrinsics, i_train, modes=None, tau=None, batcher=None, device=None):
    """Confidence.precompute_conf_map (confidence.py:78-112) on the device: for every position of i_train the maps of that image against
    its neighbours (`select_conf_neighbours`, args.conf_num) -> a list with one {mode: [H*W] fp32 device tensor} per position, keys in
    the order of `modes` (default: the list build_confidence_model forms from args; `tau` default args.tau).  An image without
    neighbours gets all-zero maps.

    images [N,H,W,3] float in [0,1] or uint8 (decoded as float32(k / 255.0): the SSIM constants are those of L = 1), depth_gts [N,H,W],
    poses [N,3,4] or [N,4,4] (bottom row 0 0 0 1), intrinsics 3x3 matrices or the batcher's [N,4] = (cx, cy, fx, fy).  With `batcher=`
    (an ImageRayBatcher) its resident tensors are used and nothing is uploaded; images / depth_gts / poses / intrinsics are then
    ignored and may be None.  args.flow or a 'vgg' mode raise NotImplementedError."""
    modes = list(modes) if modes is not None else _modes_of(args)
    if getattr(args, "flow", False):
        raise NotImplementedError(_NO_FLOW)
    if "vgg" in modes:
        raise NotImplementedError(_NO_VGG)
    bad = [m for m in modes if m not in ops.REPROJ_MODES]
    if bad or not modes or len(set(modes)) != len(modes):
        raise ValueError(f"precompute_conf_map: modes are distinct names out of {ops.REPROJ_MODES}, got {modes}")
    tau = float(tau if tau is not None else getattr(args, "tau", 0.2))
    if batcher is not None:
        img, dep, P, K = batcher.images, batcher.depths, batcher.poses, batcher.intrinsics
    else:
        from .sample_utils import _intr, _stack
        device = torch.device(device if device is not None else "cuda")
        img = _stack(images)
        img = img.to(device, torch.uint8 if img.dtype == torch.uint8 else torch.float32).contiguous()
        dep = _stack(depth_gts).to(device, torch.float32).contiguous()
        P = _stack(poses).to(device, torch.float32)[:, :3, :4].contiguous()
        K = _stack(intrinsics)
        if K.dim() == 3:
            K = torch.as_tensor(np.asarray([_intr(k) for k in K], dtype=np.float32))
        K = K.to(device, torch.float32).contiguous()
    N, H, W = (int(v) for v in img.shape[:3])
    it = [int(i) for i in np.asarray(i_train.cpu() if torch.is_tensor(i_train) else i_train).reshape(-1)]
    if not it or min(it) < 0 or max(it) >= N:
        raise ValueError("precompute_conf_map: i_train holds image indices inside [0, N)")
    out = torch.empty(len(it), len(modes), H, W, dtype=torch.float32, device=img.device)
    ws = torch.empty(ops.reproj_conf_ws(H, W), dtype=torch.uint8, device=img.device)
    for p, base in enumerate(it):
        ops.reproj_conf(img, dep, P, K, base, select_conf_neighbours(it, cam_index, p, args.conf_num), modes, tau, out=out[p], ws=ws)
    return [{m: out[p, k].reshape(-1) for k, m in enumerate(modes)} for p in range(len(it))]


class ConfidenceMaps:
    """What Confidence.precompute_conf_map returns -- a list with one {mode: [H*W] tensor} per position of i_train -- on the device:
    `maps` fp32 [M,P,H,W] in the order of `modes`, `slot_of_image` int32 [num_images] (position in i_train, or -1: the reference
    indexes the maps by that position and lambdas by the image, confidence.py:193,196) and `sky` uint8 [num_images,H,W] or None
    (args.skymask: those pixels have confidence 1, confidence.py:202-203)."""

    def __init__(self, all_conf_maps, i_train, num_images, H, W, skymask=None, device=None):
        """the modes are the keys of the first image's dict; every image's dict must hold all of them.  Maps that are device tensors
        (what `precompute_conf_map` below returns) are gathered on their device: nothing is copied to the host"""
        i_train = [int(i) for i in np.asarray(i_train).reshape(-1)]
        H, W, n = int(H), int(W), int(num_images)
        if len(all_conf_maps) != len(i_train) or not i_train:
            raise ValueError(f"ConfidenceMaps: one dict of maps per i_train position ({len(i_train)}), got {len(all_conf_maps)}")
        if len(set(i_train)) != len(i_train) or min(i_train) < 0 or max(i_train) >= n:
            raise ValueError("ConfidenceMaps: i_train holds distinct image indices inside [0, num_images)")
        self.modes = list(all_conf_maps[0].keys())
        if not 1 <= len(self.modes) <= MAX_MODES:
            raise ValueError(f"ConfidenceMaps: 1..{MAX_MODES} modes, got {len(self.modes)}")
        first = all_conf_maps[0][self.modes[0]]
        home = first.device if torch.is_tensor(first) and first.is_cuda else torch.device("cpu")
        maps = torch.empty(len(self.modes), len(i_train), H, W, dtype=torch.float32, device=home)
        for p, d in enumerate(all_conf_maps):
            for k, mode in enumerate(self.modes):
                if mode not in d:
                    raise ValueError(f"ConfidenceMaps: image {i_train[p]} (position {p}) has no '{mode}' map")
                m = torch.as_tensor(d[mode]).detach().to(home, torch.float32)
                if m.numel() != H * W:
                    raise ValueError(f"ConfidenceMaps: the '{mode}' map of image {i_train[p]} has {m.numel()} values, H * W = {H * W}")
                maps[k, p] = m.reshape(H, W)
        slot = torch.full((n,), -1, dtype=torch.int32)
        slot[torch.tensor(i_train, dtype=torch.int64)] = torch.arange(len(i_train), dtype=torch.int32)
        sky = None
        if skymask is not None:
            sky = torch.as_tensor(skymask).detach().to("cpu")
            if tuple(sky.shape) != (n, H, W):
                raise ValueError(f"ConfidenceMaps: skymask is [num_images, H, W] = {(n, H, W)}, got {tuple(sky.shape)}")
            sky = (sky != 0).to(torch.uint8).contiguous()
        self.num_images, self.H, self.W, self.i_train = n, H, W, i_train
        self.maps, self.slot_of_image, self.sky = maps, slot, sky
        self.to(device if device is not None else home)

    def to(self, device):
        self.maps, self.slot_of_image = self.maps.to(device).contiguous(), self.slot_of_image.to(device)
        self.sky = None if self.sky is None else self.sky.to(device)
        return self

    def for_model(self, conf_net):
        """-> self, after checking that the maps serve `conf_net` (every mode of the model, one column per image); the reference looks
        the maps up by mode name, so maps held in another order, or with modes the model does not mix, are brought into its order"""
        missing = [m for m in conf_net.modes if m not in self.modes]
        if missing:
            raise ValueError(f"ConfidenceMaps: the maps have no mode {missing} of the confidence model (maps: {self.modes})")
        if conf_net.lambdas.shape[1] != self.num_images:
            raise ValueError(f"ConfidenceMaps: maps for {self.num_images} images, the confidence model has {conf_net.lambdas.shape[1]} columns")
        if list(conf_net.modes) != self.modes:
            self.maps = self.maps[[self.modes.index(m) for m in conf_net.modes]].contiguous()
            self.modes = list(conf_net.modes)
        return self


class _FinalConfidence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lambdas, maps, sel_coords, img_i):
        ctx.maps, ctx.coords, ctx.img = maps, sel_coords, img_i
        ctx.save_for_backward(lambdas)
        return ops.conf_apply(maps.maps, maps.slot_of_image, lambdas.detach(), maps.sky, img_i, sel_coords)

    @staticmethod
    def backward(ctx, g_conf):
        lambdas, = ctx.saved_tensors
        maps = ctx.maps
        grad = torch.zeros_like(lambdas)
        ops.conf_grad(maps.maps, maps.slot_of_image, lambdas.detach(), maps.sky, ctx.img, ctx.coords, g_conf.contiguous(), grad)
        return grad, None, None, None


def calc_final_confidence(conf_net, maps, sel_coords, img_i):
    """The precomputed branch of calc_final_confidence (confidence.py:193-206) for every ray of the batch, differentiable in
    conf_net.lambdas: sel_coords int64 [n,2] = (row, col) on the device, img_i a python int or an int64 [1] device tensor -> conf [n].
    (The reference then keeps the rays with a depth target, `[target_mask]`; multiply the per-ray depth loss of all rays instead.)"""
    maps.for_model(conf_net)
    return _FinalConfidence.apply(conf_net.lambdas, maps, sel_coords.contiguous(), img_i)


def conf_sums(maps, sky, g_conf):
    """the float64 sums snerf_conf_grad forms over a batch: maps [M,n] (the map values at the rays' pixels), sky [n] (bool, or None),
    g_conf [n] -> A [M]"""
    f = lambda x: torch.as_tensor(x).detach().cpu().to(torch.float64)
    g = f(g_conf)
    if sky is not None:
        g = g * (~torch.as_tensor(sky).detach().cpu().bool()).to(torch.float64)
    return f(maps) @ g


def conf_grad_chain(lam, A):
    """Host model of snerf_conf_grad's chain, float64: lam [M] (one table column), A [M] (conf_sums) -> d loss / d lam [M]:
    d lam_k = s_k (1 - s_k) / S (A_k - sum_j s_j A_j / S) with s = sigmoid(lam), S = sum s."""
    lam = torch.as_tensor(lam).detach().cpu().to(torch.float64).reshape(-1)
    A = torch.as_tensor(A, dtype=torch.float64).reshape(-1)
    s = 1.0 / (1.0 + torch.exp(-lam))
    S = s.sum()
    return s * (1.0 - s) / S * (A - (s * A).sum() / S)
