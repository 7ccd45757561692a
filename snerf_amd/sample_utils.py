"""Ray generation on the device: host-side mirror of s-nerf/utils/sample_utils.py (the step immediately before the render
path).  Same function names and argument meaning as the reference; the per-pixel arithmetic runs in
`snerf_pinhole_rays` (no [H, W, 3] direction grid is materialised to pick 4096 pixels).  `args` needs `no_ndc=True` (the
S-NeRF street-scene configuration); NDC rays raise NotImplementedError."""
import collections

import numpy as np
import torch

from . import ops
from .batching import DrawCounter, shard_bounds

Rays = collections.namedtuple('Rays', ('origins', 'directions', 'viewdirs', 'radii', 'lossmult', 'near', 'far', 'app'))


def _intr(intrinsic):
    K = np.asarray(intrinsic.detach().cpu() if torch.is_tensor(intrinsic) else intrinsic, dtype=np.float32)
    return float(K[0, 2]), float(K[1, 2]), float(K[0, 0]), float(K[1, 1])


def _pose(pose):
    return np.asarray(pose.detach().cpu() if torch.is_tensor(pose) else pose, dtype=np.float32)


def _check(args):
    if not getattr(args, "no_ndc", True):
        raise NotImplementedError("NDC rays (no_ndc=False) are outside the accelerated path")


def get_rays_single_img(args, image, depth_gt, pose, intrinsic, near=0., far=1., factor=4, device=None):
    """sample_utils.py:286-345: rays of the whole (H//factor x W//factor) frame -> Rays with [H, W, .] fields."""
    _check(args)
    H, W = image.shape[0] // factor, image.shape[1] // factor
    device = device if device is not None else (image.device if torch.is_tensor(image) and image.is_cuda else torch.device("cuda"))
    cx, cy, fx, fy = (v / factor for v in _intr(intrinsic))
    # float32 arithmetic of `intrinsic / factor` (sample_utils.py:290)
    cx, cy, fx, fy = (float(np.float32(v)) for v in (cx, cy, fx, fy))
    o, d, v, r, nr, fr = ops.pinhole_rays(None, 0, H * W, W, H, _pose(pose), cx, cy, fx, fy, False, near * 0.9, far * 1.1, device)
    ones = torch.ones(H, W, 1, dtype=torch.float32, device=device)
    sh = lambda t: t.view(H, W, -1)
    return Rays(sh(o), sh(d), sh(v), sh(r), ones, sh(nr), sh(fr), ones * 0.)


def rays_of_pixels(coords, pose, intrinsic, H, W, near, far, training=False, device="cuda"):
    """Rays of selected pixels; coords [N,2] = (row, col) (any integer tensor / array)."""
    c = torch.as_tensor(coords).to(device=device, dtype=torch.int32).contiguous()
    cx, cy, fx, fy = _intr(intrinsic)
    o, d, v, r, nr, fr = ops.pinhole_rays(c, 0, c.shape[0], W, H, _pose(pose), cx, cy, fx, fy, training, near, far, device)
    ones = torch.ones_like(r)
    return Rays(o, d, v, r, ones, nr, fr, ones * 0.)


def sample_patches(H, W, patch_sz, n_patch):
    """sample_utils.py:68-89 (sample_patches_pt): `n_patch` centres drawn with np.random.randint among the pixels strictly more than `patch_sz` from
    every border (row-major order of that window), each giving the (2 (patch_sz // 2))^2 pixels [c - patch_sz // 2, c + patch_sz // 2) around it,
    rows outer.  -> int64 [n_patch * (2 (patch_sz // 2))^2, 2] of (row, col)."""
    hr, wc = H - 2 * patch_sz - 1, W - 2 * patch_sz - 1                  # rows / columns r with patch_sz < r < H - patch_sz
    if hr <= 0 or wc <= 0:
        raise ValueError("image smaller than the smooth-loss patch margin (the reference's np.random.randint(0) raises here too)")
    idx = np.random.randint(hr * wc, size=n_patch)
    return patch_pixels(np.stack([patch_sz + 1 + idx // wc, patch_sz + 1 + idx % wc], -1), patch_sz)


def smooth_loss(image, skymask, sel_coords_smooth, pred_distance_smooth, n_patch, patch_sz, weight, use_skymask=True):
    """loss_factory.py:38-57 (SmoothLoss) on loss.py:14-35 (edge_aware_loss_v2): the edge-aware smoothness of the patches' disparities, in torch
    ops (autograd carries it to `pred_distance_smooth` = the renderer's distances of the batch's patch rays, train.py:154-177).  A caller-side
    loss: off in the shipped config (configs/nuScenes_depth_6cams:61), no kernel."""
    img = torch.as_tensor(image)
    c = torch.as_tensor(sel_coords_smooth).long().to(img.device)
    dev = pred_distance_smooth.device
    rgb = img[c[:, 0], c[:, 1]].to(dev).view(n_patch, patch_sz, patch_sz, -1)
    disp = (1 / torch.clamp(pred_distance_smooth, min=1e-5)).view(n_patch, patch_sz, patch_sz, -1)
    disp = disp / (disp.mean(1, True).mean(2, True) + 1e-7)
    gx = torch.abs(disp[:, :, :-1, :] - disp[:, :, 1:, :]) * torch.exp(-torch.mean(torch.abs(rgb[:, :, :-1, :] - rgb[:, :, 1:, :]), 3, keepdim=True))
    gy = torch.abs(disp[:, :-1, :, :] - disp[:, 1:, :, :]) * torch.exp(-torch.mean(torch.abs(rgb[:, :-1, :, :] - rgb[:, 1:, :, :]), 3, keepdim=True))
    if use_skymask:
        sky = torch.as_tensor(skymask)[c[:, 0].to(torch.as_tensor(skymask).device), c[:, 1].to(torch.as_tensor(skymask).device)].to(dev).view(n_patch, patch_sz, patch_sz, -1)
        gx = gx + sky[:, :, :-1, :] * gx
        gy = gy + sky[:, :-1, :, :] * gy
    return (gx.mean() + gy.mean()) * weight


def sample_single_img(args, image, depth_gt, pose, intrinsic, near=0., far=1., near_far=False, batch_n=None, app=0.):
    """sample_utils.py:92-211: a random pixel batch of one image -> (Rays, target_rgb, target_depth, sel_coords, sel_inds).
    The pixel choice uses numpy's global RNG exactly like the reference (np.random.choice without replacement)."""
    _check(args)
    H, W = image.shape[:2]
    n = batch_n if batch_n is not None else args.N_rgb
    patches = None
    if getattr(args, "smooth_loss", False):
        # --smooth_loss (sample_utils.py:102-103, 136-138): N_patch random patches appended BEHIND the random pixels; their centres are drawn first
        patches = sample_patches(H, W, int(args.patch_sz), int(args.N_patch))
    sel = np.random.choice(H * W, size=[n], replace=False)
    coords = np.stack([sel // W, sel % W], -1)
    if patches is not None:
        coords = np.concatenate([coords, patches], 0)
    if not near_far:
        near, far = near * 0.9, far * 1.1
    else:
        nz = depth_gt[depth_gt != 0]
        near, far = float(nz.min()) * 0.9, float(nz.max()) * 1.1
    dev = image.device if torch.is_tensor(image) and image.is_cuda else torch.device("cuda")
    rays = rays_of_pixels(coords, pose, intrinsic, H, W, near, far, training=True, device=dev)
    rays = rays._replace(app=rays.lossmult * float(app))
    ct = torch.as_tensor(coords, device=image.device if torch.is_tensor(image) else "cpu").long()
    target_rgb = image[ct[:, 0], ct[:, 1]]
    target_dep = depth_gt[ct[:, 0], ct[:, 1]]
    return rays, target_rgb, target_dep, ct, sel


def apply_pose_transform(rays, pose):
    """The pose-refinement half of `sample_rays` (sample_utils.py:421-435): rotate directions / viewdirs by pose[:3, :3] and shift the
    origins by pose[:3, 3], in torch, so that autograd links the rays to a learnable pose (`pose = pose_param_net(img_i,
    transform_only=True)`).  The rays this module generates are detached from any pose tensor (the per-pixel arithmetic runs in a
    kernel); with `pose.requires_grad` the returned origins / directions / viewdirs require grad, `MipNerfModel` / zipnerf `Model`
    deliver d loss / d rays for them, and `loss.backward()` reaches the pose parameters as in the reference."""
    R, t = pose[:3, :3], pose[:3, 3]
    rot = lambda v: (v[..., None, :] * R).sum(-1)
    return rays._replace(origins=rays.origins + t, directions=rot(rays.directions), viewdirs=rot(rays.viewdirs))


# ---- device-resident training batcher (snerf_mip_image_batch) ------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def philox(c, seed):
    """Philox4x32-10 of the 4-word counter `c` under the 64-bit `seed` -> its first output word (host form of csrc/callers.hip's)."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in c)
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0


def keyed_perm(v, M, tag, t, seed):
    """The keyed permutation of [0, M) the batchers draw with (4-round Feistel network with cycle walking; csrc/callers.hip)."""
    b = max(2, (M - 1).bit_length())
    b += b & 1
    h = b >> 1
    mask = (1 << h) - 1
    t &= (1 << 64) - 1
    while True:
        for j in range(4):
            L, R = v >> h, v & mask
            v = (R << h) | (L ^ (philox((R, tag << 16 | j, t & _M32, t >> 32), seed) & mask))
        if v < M:
            return v


CLASSIC_BATCH_TAG = 4                                # keyed_perm tag of classic.RayBatcher (1 / 2: ImageRayBatcher's image and pixel orders, 3: the bounded draws)


def classic_rays_of_step(s, n_rand, T, seed, rank=0, world=1):
    """classic.RayBatcher's schedule (host form of snerf_classic_train_batch): the ray indices in [0, T) of rank's rows of step s.  Row r of
    the global batch sits at position p = s n_rand + r of the endless ray stream, in epoch e = p // T, and is ray
    keyed_perm(p % T, T, CLASSIC_BATCH_TAG, e, seed): every epoch visits each of the T rays once, in an order of its own; a batch may
    straddle an epoch boundary.  -> int64 [rows of shard_bounds(n_rand, rank, world)]"""
    i0, i1 = shard_bounds(int(n_rand), int(rank), int(world))
    out = np.empty(i1 - i0, dtype=np.int64)
    for k, r in enumerate(range(i0, i1)):
        e, pos = divmod(int(s) * int(n_rand) + r, int(T))
        out[k] = keyed_perm(pos, int(T), CLASSIC_BATCH_TAG, e, int(seed))
    return out


def image_of_step(i_train, seed, s):
    """ImageRayBatcher's image schedule: step s of epoch e = s // len(i_train) trains on i_train[keyed_perm(s % len(i_train))] (each
    training image once per epoch, a new order every epoch)."""
    nt = len(i_train)
    e, p = divmod(int(s), nt)
    return int(i_train[keyed_perm(p, nt, 1, e, int(seed))])


def bounded_draw(i, v, s, rng, seed):
    """Lemire's unbiased integer in [0, rng) the batchers draw with: attempts a = 0, 1, ... on the counter (i, 3 << 16 | v << 8 | a,
    lo32(s), hi32(s)), attempt 255 accepted as it is (csrc/callers.hip)."""
    thresh = ((1 << 32) - rng) % rng
    s &= (1 << 64) - 1
    for a in range(256):
        m = philox((i, 3 << 16 | v << 8 | a, s & _M32, s >> 32), seed) * rng
        if (m & _M32) >= thresh:
            break
    return m >> 32


def _patch_window(H, W, patch_sz):
    """rows / columns of sample_patches' centre window: the pixels r with patch_sz < r < H - patch_sz (and the same in W)"""
    return H - 2 * patch_sz - 1, W - 2 * patch_sz - 1


def patch_centres_of_step(s, seed, H, W, patch_sz, n_patch):
    """PatchRayBatcher's patch schedule: centre k of step s = bounded_draw(k, 3, s, hr wc) over the hr x wc pixels of sample_patches'
    window in row-major order (with replacement, like np.random.randint there) -> int64 [n_patch, 2] of (row, col)."""
    hr, wc = _patch_window(int(H), int(W), int(patch_sz))
    if hr <= 0 or wc <= 0:
        raise ValueError("image smaller than the smooth-loss patch margin")
    idx = np.asarray([bounded_draw(k, 3, int(s), hr * wc, int(seed)) for k in range(int(n_patch))], dtype=np.int64).reshape(-1)
    return np.stack([patch_sz + 1 + idx // wc, patch_sz + 1 + idx % wc], -1).astype(np.int64)


def patch_pixels(centres, patch_sz):
    """the pixels of the patches around `centres` [k, 2]: [c - patch_sz // 2, c + patch_sz // 2) in both axes, rows outer, patches in order
    (the layout half of sample_patches) -> int64 [k (2 (patch_sz // 2))^2, 2] of (row, col)."""
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 2)
    h = patch_sz // 2
    dr, dc = np.meshgrid(np.arange(-h, h), np.arange(-h, h), indexing="ij")
    rows = (c[:, 0, None, None] + dr[None]).reshape(-1)
    cols = (c[:, 1, None, None] + dc[None]).reshape(-1)
    return np.stack([rows, cols], -1).astype(np.int64)


def _stack(x, dtype=None):
    if torch.is_tensor(x):
        return x.detach()
    if isinstance(x, (list, tuple)):
        return torch.stack([torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v) for v in x])
    return torch.as_tensor(np.asarray(x, dtype=dtype) if dtype is not None else np.asarray(x))


class ImageRayBatcher(DrawCounter):
    """Device-resident form of SingleImage + sample_single_img (s-nerf/dataloader/rayset.py:124-151, the `no_batching` loader that
    `pose_refine = True` selects): the training images, depth maps, poses and intrinsics live on the device and `next()` draws, casts and
    gathers one batch in ONE launch (`snerf_mip_image_batch`), with no host work, no upload and no sync per step.

    Step s trains on image `image_of_step(s)` (a keyed permutation of i_train per epoch: DataLoader(shuffle=True, batch_size=1)
    semantics) and on batch_n distinct pixels of it (without replacement, like np.random.choice(H W, n, replace=False)).  Only that
    draw differs from the reference (a counter-based generator keyed by `seed` instead of numpy's); given the pixels, rays, targets
    and bounds are what sample_single_img returns, bit for bit: near / far are near * 0.9 / far * 1.1, or with args.near_far the
    image's non-zero depth float(min) * 0.9 / float(max) * 1.1 (computed once here), app = camera_index[img].

    Rank r of `world` computes rows shard_bounds(batch_n, r, world) of the one global batch: the ranks together see exactly the rays of
    a single-GPU run.  images: [N,H,W,3] uint8 (decoded to float32(k / 255.0)) or float; extras: per-pixel fp32 maps [N,H,W]
    (confidence maps, sky masks) gathered with the targets."""

    draws_patches = False                            # (PatchRayBatcher: the --smooth_loss patches behind the random pixels)

    def __init__(self, args, images, depth_gts, poses, intrinsics, i_train, near, far, camera_index=None, batch_n=None, extras=None, seed=0,
                 rank=0, world=1, device=None):
        _check(args)
        if getattr(args, "smooth_loss", False) and not self.draws_patches:
            raise NotImplementedError("smooth_loss: ImageRayBatcher draws no patches; PatchRayBatcher does")
        img = _stack(images)
        if img.dim() != 4 or img.shape[-1] != 3 or img.shape[0] == 0:
            raise ValueError("images: [N, H, W, 3] with N >= 1")
        N, H, W = (int(v) for v in img.shape[:3])
        n = int(batch_n if batch_n is not None else args.N_rgb)
        if not 0 < n <= H * W:
            raise ValueError(f"batch_n = {n}: needs 0 < batch_n <= H W = {H * W} (pixels are drawn without replacement)")
        if H < 3:
            raise ValueError("images need at least 3 rows (the radius of the last row is that of row H - 3)")
        it = np.asarray(i_train.cpu() if torch.is_tensor(i_train) else i_train, dtype=np.int64).reshape(-1)
        if it.size == 0:
            raise ValueError("i_train is empty")
        if it.min() < 0 or it.max() >= N:
            raise ValueError("i_train indexes past the images")
        dep = _stack(depth_gts).to(torch.float32)
        if tuple(dep.shape) != (N, H, W):
            raise ValueError(f"depth_gts: [N, H, W] = {(N, H, W)}, got {tuple(dep.shape)}")
        P = _stack(poses).to(torch.float32)[:, :3, :4]
        K = [_intr(k) for k in (_stack(intrinsics))]
        if P.shape[0] != N or len(K) != N:
            raise ValueError("poses / intrinsics: one per image")
        ex = None
        if extras is not None and len(extras) > 0:
            ex = torch.stack([_stack(e).to(torch.float32) for e in extras])
            if tuple(ex.shape[1:]) != (N, H, W):
                raise ValueError("extras: per-pixel maps [N, H, W]")
        if getattr(args, "near_far", False):
            # sample_single_img's near_far bounds, per training image (one device->host read here, none per step)
            bounds = {}
            for i in sorted(set(it.tolist())):
                nz = dep[i][dep[i] != 0]
                bounds[i] = (float(nz.min()) * 0.9, float(nz.max()) * 1.1)
            nf = [bounds.get(i, (near * 0.9, far * 1.1)) for i in range(N)]
        else:
            nf = [(near * 0.9, far * 1.1)] * N
        cam = np.zeros(N) if camera_index is None else np.asarray(camera_index.cpu() if torch.is_tensor(camera_index) else camera_index, dtype=np.float64).reshape(-1)
        super().__init__(n, seed, rank, world, device)                          # (the last check; the first thing on the device)
        device = self.device
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        self.images = img.to(device, torch.uint8 if img.dtype == torch.uint8 else torch.float32).contiguous()
        self.depths = dep.to(device).contiguous()
        self.poses, self.intrinsics = P.to(device).contiguous(), f32(K)
        self.near_img, self.far_img = [b[0] for b in nf], [b[1] for b in nf]   # the bounds sample_single_img passes on (python floats)
        self.near, self.far, self.app = f32(self.near_img), f32(self.far_img), f32([float(cam[i]) for i in range(N)])
        self.extras = None if ex is None else ex.to(device).contiguous()
        self.i_train_host = it
        self.i_train = torch.as_tensor(it, dtype=torch.int32).to(device)
        self.N, self.H, self.W, self.batch_n = N, H, W, n

    def image_of_step(self, s):
        """index (into the images) of the image step s trains on -- on the host, no sync (pose refinement: pose_param_net(img_i))"""
        return image_of_step(self.i_train_host, self.seed, s)

    def buffers(self):
        """fresh output tensors of one batch (this rank's rows)"""
        m, dev = self.n_rows, self.device
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        return dict(origins=e(m, 3), directions=e(m, 3), viewdirs=e(m, 3), radii=e(m, 1), lossmult=e(m, 1), near=e(m, 1), far=e(m, 1),
                    app=e(m, 1), rgb=e(m, 3), depth=e(m), extras=None if self.extras is None else e(self.extras.shape[0], m),
                    sel_coords=e(m, 2, dt=torch.int64), img=e(1, dt=torch.int64))

    def next_into(self, buf):
        """draw the next batch into `buf` (from `buffers()`) on the current stream; graph-capturable (every replay draws the next step)
        -> (rays, target_rgb, target_depth, sel_coords, img_i, extras) as views of `buf`"""
        ops.mip_image_batch(self.images, self.depths, self.poses, self.intrinsics, self.near, self.far, self.app, self.extras, self.i_train,
                            self.seed, self.counter, self.batch_n, self.i0, self.i1, buf)
        return self._drawn(self.view(buf))

    @staticmethod
    def view(buf):
        rays = Rays(buf["origins"], buf["directions"], buf["viewdirs"], buf["radii"], buf["lossmult"], buf["near"], buf["far"], buf["app"])
        ex = [] if buf["extras"] is None else list(buf["extras"].unbind(0))
        return rays, buf["rgb"], buf["depth"], buf["sel_coords"], buf["img"], ex


class PatchRayBatcher(ImageRayBatcher):
    """ImageRayBatcher for --smooth_loss configs (sample_utils.py:102-103,136-138): every batch is the batch_n random pixels of the
    step's image followed by n_patch patches of patch_sz x patch_sz pixels of the same image, drawn, cast and gathered by the same ONE
    launch (`snerf_mip_image_patch_batch`).  The image and the random pixels are those an ImageRayBatcher of the same seed draws at the
    same step; the patch centres are `patch_centres_of_step(step, seed, H, W, patch_sz, n_patch)` -- with replacement over the pixels
    strictly more than patch_sz from every border, the window of `sample_patches` -- and their pixels `patch_pixels(centres, patch_sz)`.
    Every field of a patch row (rays, rgb, depth, extras, sel_coords, bounds, app) is what a pixel row of that pixel holds.

    Rank r of `world` takes pixel rows shard_bounds(batch_n, r, world) and WHOLE patches shard_bounds(n_patch, r, world) (a rank may
    get none): `n_rgb_rows` pixel rows in front of `n_patch_rows` patch rows.  MipTrainer.step(..., n_rgb=batcher.n_rgb_rows) trains on
    it; the ranks' pixel rows and patches together are those of a single-GPU run."""
    draws_patches = True

    def __init__(self, args, images, depth_gts, poses, intrinsics, i_train, near, far, camera_index=None, batch_n=None, extras=None, seed=0,
                 rank=0, world=1, device=None, n_patch=None, patch_sz=None):
        n_patch = int(n_patch if n_patch is not None else args.N_patch)
        p = int(patch_sz if patch_sz is not None else args.patch_sz)
        if n_patch < 1:
            raise ValueError(f"n_patch = {n_patch}: a PatchRayBatcher draws at least one patch (ImageRayBatcher draws none)")
        if p < 2 or p > 32 or p % 2:
            raise ValueError(f"patch_sz = {p}: an even size in 2..32 (the patch is [c - patch_sz // 2, c + patch_sz // 2) around its centre)")
        shape = _stack(images).shape
        if len(shape) == 4:
            hr, wc = _patch_window(int(shape[1]), int(shape[2]), p)
            if hr < 1 or wc < 1 or hr * wc >= 1 << 32:
                raise ValueError(f"images of {int(shape[1])} x {int(shape[2])} leave no pixel more than patch_sz = {p} from every border "
                                 "(or 2^32 and more of them)")
        super().__init__(args, images, depth_gts, poses, intrinsics, i_train, near, far, camera_index=camera_index, batch_n=batch_n,
                         extras=extras, seed=seed, rank=rank, world=world, device=device)
        self.n_patch, self.patch_sz = n_patch, p
        self.k0, self.k1 = shard_bounds(n_patch, self.rank, self.world)

    @property
    def n_rgb_rows(self):
        """this rank's pixel rows: the rows in front of its patch rows (MipTrainer.step's n_rgb)"""
        return self.i1 - self.i0

    @property
    def n_patch_rows(self):
        """this rank's patch rows: its whole patches times patch_sz^2"""
        return (self.k1 - self.k0) * self.patch_sz ** 2

    @property
    def n_rows(self):
        return self.n_rgb_rows + self.n_patch_rows

    def patch_centres_of_step(self, s):
        """the n_patch centres of step s, int64 [n_patch, 2] -- on the host, no sync (this rank's are rows [k0, k1))"""
        return patch_centres_of_step(s, self.seed, self.H, self.W, self.patch_sz, self.n_patch)

    def next_into(self, buf):
        ops.mip_image_patch_batch(self.images, self.depths, self.poses, self.intrinsics, self.near, self.far, self.app, self.extras,
                                  self.i_train, self.seed, self.counter, self.batch_n, self.i0, self.i1, self.n_patch, self.patch_sz,
                                  self.k0, self.k1, buf)
        return self._drawn(self.view(buf))
