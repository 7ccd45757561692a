"""Reprojection confidence maps on the device: snerf_reproj_conf / ops.reproj_conf, confidence.select_conf_neighbours,
confidence.precompute_conf_map and ConfidenceMaps on device tensors.

The yardstick is the reference's own text, restated once below in torch and evaluated in float64 on the CPU: precompute_conf_map and
select_conf_depends (s-nerf/model/confidence.py:78-169), warping and sample_points (model/loss.py:122-179), reproj_err (:218-268),
get_reproj_conf (:271-327) and ssim (utils/pytorch_msssim/__init__.py:7-60).  test_restatement_is_the_reference pins it to the imported
reference.  Two things the reference leaves open are defined as the kernels define them: a pass with no pixel in view is skipped (the
reference raises on the empty max) and the in-view test is made on the rounded floats (a non-finite coordinate is out of view).

Discrete events are a condition of the scenes, not a tolerance: a projection within 2e-4 px of a rounding tie in u or v may flip the
mask or the nearest-depth texel in fp32 (and with it SSIM over an 11 x 11 neighbourhood), and a depth error next to tau may flip the
depth mask.  The seeds below were found by a CPU search so that no pixel of any pass is that close in float64; the tests assert it and
exclude no pixel from any comparison.

The tolerance is not a fixed number: d_mode = max |restatement in fp32 - restatement in float64| is the reference's own arithmetic
noise on the scene, and the kernel must be within max(4 d_mode, 16 * 2^-24) of the float64 restatement on every pixel (4: the window
is applied separably and the sums run in another order than conv2d's; floor: maps in [0,1] after about a dozen roundings)."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from snerf_amd import _lib, confidence, ops

gpu = pytest.mark.gpu
EPS = 2.0 ** -24
REF = "/root/reference/s-nerf"
ALL_MODES = ("rgb", "ssim", "depth")
TAU = float(torch.tensor(0.2, dtype=torch.float32))     # tau as the fp32 value the kernels receive
TIE = 2e-4                                              # px: no projection may be this close to a rounding tie (float64)
TAU_GAP = 1e-4                                          # no in-view depth error may be this close to tau (float64)
# name -> (H, W, cam_index, i_train, conf_num, seed); the seeds satisfy the precondition above (found by a CPU search over seeds)
SCENES = {"main": (24, 40, (0, 0, 0, 1), (0, 1, 2, 3), 2, 121), "tiles": (45, 70, (0, 0, 0), (0, 1, 2), 1, 254)}


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_window(dt):
    """pytorch_msssim gaussian + create_window (:7-16): the fp32 outer product of the normalised fp32 1-D window, for 3 channels"""
    gauss = torch.Tensor([np.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])                   # :8
    w1 = (gauss / gauss.sum()).unsqueeze(1)                                                                        # :9,13
    return w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(3, 1, 11, 11).contiguous().to(dt)                # :14-15


def ref_ssim(img1, img2):
    """ssim(full=True) (:19-60) with L = 1 (images in [0,1]: max <= 128, min >= -0.5) -> ssim_map [1,3,H,W]"""
    window = ref_window(img1.dtype)
    conv = lambda x: F.conv2d(x, window, padding=5, groups=3)                                                      # :40-41
    mu1, mu2 = conv(img1), conv(img2)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2                                                    # :43-45
    sigma1_sq, sigma2_sq, sigma12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2   # :47-49
    C1, C2 = (0.01 * 1) ** 2, (0.03 * 1) ** 2                                                                      # :51-52
    v1, v2 = 2.0 * sigma12 + C2, sigma1_sq + sigma2_sq + C2                                                        # :54-55
    return ((2 * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2)                                               # :58


def ref_warping(S, base, tgt):
    """warping (loss.py:138-179) + sample_points (:122-135) in S's dtype -> fake_img [H,W,3], tgt_depth [n], fake_depth [n],
    mask [H*W] and the projected coordinates (u, v) of every pixel"""
    img, dep, pose, K = S["images"], S["depths"], S["poses"], S["intr"]
    H, W = img.shape[1:3]
    dt = img.dtype
    proj_coord = torch.flip(torch.nonzero(torch.ones((H, W))), [1])                            # confidence.py:92-93: (x = col, y = row)
    base_intr, tgt_intr = K[base], K[tgt]
    focal = torch.stack([base_intr[0][0], base_intr[1][1]]).mean()                             # :146
    tgt_focal = torch.stack([tgt_intr[0][0], tgt_intr[1][1]]).mean()                           # :147
    i, j = (proj_coord[:, 0] - base_intr[0, 2]) / focal, -(proj_coord[:, 1] - base_intr[1, 2]) / focal            # :148
    dirs = torch.stack([i, j, -torch.ones_like(i)], -1).permute(1, 0) * dep[base].reshape(-1, 1)[:, 0]             # :150
    dirs = F.pad(dirs.permute(1, 0), (0, 1), "constant", 1).to(dt)                                                 # :151
    pts = pose[base] @ dirs.T                                                                                      # :153
    tgt_cam_pt = (torch.inverse(pose[tgt]) @ pts)[:3].T                                                            # :154
    depth = tgt_cam_pt[:, 2].clone().abs()                                                                         # :156
    tgt_coord = torch.stack([tgt_cam_pt[:, 0] / depth, tgt_cam_pt[:, 1] / depth], -1) * tgt_focal                  # :157-159
    tgt_coord = torch.stack([tgt_coord[:, 0] + tgt_intr[0, 2], -tgt_coord[:, 1] + tgt_intr[1, 2]], -1)             # :160-161
    xr, yr = tgt_coord[:, 1].round(), tgt_coord[:, 0].round()                                                      # :163 (half to even)
    mask = (xr >= 0) & (xr < H) & (yr >= 0) & (yr < W)                                                             # :166-168, on the floats
    x, y = xr[mask].long(), yr[mask].long()
    grid = tgt_coord[mask].clone()                                                                                 # sample_points :127
    grid = torch.stack([grid[:, 0] / ((W - 1) // 2) - 1, grid[:, 1] / ((H - 1) // 2) - 1], -1)                     # :129-130
    sample_rgb = F.grid_sample(img[tgt].unsqueeze(0).permute(0, 3, 1, 2), grid[None, ...].unsqueeze(2), align_corners=False)   # :133
    sample_rgb = sample_rgb.squeeze(3).squeeze(0).T
    fake_img = torch.zeros_like(img[base])                                                                         # :175
    coord = proj_coord[mask]
    fake_img[coord[:, 1], coord[:, 0]] = sample_rgb                                                                # :177
    return fake_img, dep[tgt][x, y], depth[mask], mask, tgt_coord


def ref_conf_maps(S, base, neighbours, modes, tau):
    """get_reproj_conf (loss.py:271-327) over reproj_err (:218-268) for one base image -> ({mode: [H*W]}, diagnostics per pass)"""
    img = S["images"]
    H, W = img.shape[1:3]
    dt = img.dtype
    confs = {m: torch.zeros(H * W, dtype=dt) for m in modes}                                   # :281
    masks = {m: torch.zeros(H * W, dtype=dt) for m in modes}                                   # :282
    depth_mask, Mask, diag = None, None, []
    for tgt in neighbours:                                                                     # :286
        fake_img, tgt_depth, fake_depth, mask, uv = ref_warping(S, base, tgt)                  # :237
        fin = torch.isfinite(uv)
        tie = ((uv - torch.floor(uv) - 0.5).abs())[fin]
        d = dict(base=base, tgt=tgt, n_in_view=int(mask.sum()), tie=float(tie.min()) if tie.numel() else 1.0, range={}, tau_gap=1.0)
        diag.append(d)
        if not bool(mask.any()):                                                               # defined here: an empty pass is skipped
            continue
        mask2 = mask.reshape(H, W)
        base_img_ = img[base].clone()                                                          # :239
        base_img_[~mask2] = 0                                                                  # :241
        err_dict = {}
        if "rgb" in modes:
            err_dict["rgb"] = (base_img_ - fake_img).abs().mean(2)[mask2].reshape(1, -1)[0]    # :245-247
        if "ssim" in modes:
            ssim_map = ref_ssim(base_img_[None, ...].permute(0, 3, 1, 2), fake_img[None, ...].permute(0, 3, 1, 2))     # :250
            err_dict["ssim"] = (1 - ssim_map.mean(1))[0][mask2].reshape(1, -1)[0]              # :251-253
        if "depth" in modes:
            err_dict["depth"] = (fake_depth - tgt_depth).abs() / torch.max(tgt_depth, torch.tensor(1e-10, dtype=dt))   # :256
        Mask = mask                                                                            # :293
        for mode in modes:                                                                     # :294
            if mode == "depth":
                d["tau_gap"] = float((err_dict["depth"] - tau).abs().min())
                depth_mask = err_dict["depth"] > tau                                           # :297
                err_dict["depth"] = torch.clamp(err_dict["depth"], max=tau)                    # :298
            conf = err_dict[mode].max() - err_dict[mode]                                       # :300
            d["range"][mode] = float(conf.max())
            conf = conf / conf.max()                                                           # :301
            confs[mode][Mask] += conf                                                          # :302
            masks[mode][Mask] += 1                                                             # :303
    for mode in modes:                                                                         # :317
        mask = masks[mode]
        mask[mask == 0] = 1                                                                    # :320
        confs[mode] = confs[mode] / mask                                                       # :321
        if depth_mask is not None:                                                             # :323-326: the LAST pass's masks only
            temp = confs[mode][Mask]
            temp[depth_mask] = 0.
            confs[mode][Mask] = temp
    return confs, diag


def ref_select(i_train, cam_index, img_i, conf_num):
    """sel_ids of select_conf_depends (confidence.py:125-135)"""
    i_train = np.asarray(i_train)
    img_idx = np.where(i_train == img_i)[0].item()                                             # :125
    sel_ids = []
    for k in range(1, conf_num + 1):                                                           # :128
        if img_idx + k < len(i_train):
            if cam_index[i_train[img_idx]] == cam_index[i_train[img_idx + k]]:
                sel_ids.append(int(i_train[img_idx + k]))
        if img_idx - k >= 0:
            if cam_index[i_train[img_idx]] == cam_index[i_train[img_idx - k]]:
                sel_ids.append(int(i_train[img_idx - k]))
    return sel_ids


def ref_precompute(S, cam_index, i_train, conf_num, modes, tau):
    """precompute_conf_map (confidence.py:78-85) -> (list of {mode: [H*W]}, the passes' diagnostics)"""
    out, diag = [], []
    for img_i in i_train:
        maps, d = ref_conf_maps(S, img_i, ref_select(i_train, cam_index, img_i, conf_num), modes, tau)
        out.append(maps)
        diag += d
    return out, diag


def ref_final_confidence(lambdas, modes, all_conf_maps, i_train, img_i, sel_coords, H, W):
    """the precomputed branch of calc_final_confidence (confidence.py:193-206) without a sky mask, float64"""
    conf_maps = all_conf_maps[np.where(np.asarray(i_train) == img_i)[0].item()]                # :193
    final_conf_map = torch.zeros((H, W), dtype=torch.float64)                                  # :195
    weights = torch.sigmoid(lambdas[:, img_i].to(torch.float64))                               # :196
    for idx, mode in enumerate(modes):                                                         # :197-198
        final_conf_map = final_conf_map + weights[idx] * conf_maps[mode].to(torch.float64).reshape(H, W)
    final_conf_map = final_conf_map / weights.sum()                                            # :199
    return final_conf_map[sel_coords[:, 0], sel_coords[:, 1]]                                  # :205


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------
def make_scene(H, W, n_img, seed):
    """fp32 tensors: smooth textured images plus noise in [0,1], depths of 8-13 with about 10 % zeros, rigid camera-to-world poses that
    step sideways and yaw by a few hundredths of a radian, slightly different intrinsics per image with fx != fy"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    images, depths, poses, intr = [], [], [], []
    for k in range(n_img):
        ph = r(3, 4) * 6.28
        tex = torch.stack([0.5 + 0.2 * torch.sin(0.31 * (xs + 1.2 * k) + ph[c, 0]) * torch.cos(0.27 * ys + ph[c, 1]) +
                           0.15 * torch.sin(0.11 * (xs + 1.2 * k) + 0.17 * ys + ph[c, 2]) for c in range(3)], -1)
        images.append((tex + 0.06 * (r(H, W, 3) - 0.5)).clamp(0, 1))
        d = 10.5 + 2.0 * torch.sin(0.09 * xs + 0.4 * k + ph[0, 3]) * torch.cos(0.07 * ys + ph[1, 3]) + 0.5 * (r(H, W) - 0.5)
        d = torch.where(r(H, W) < 0.08, d * (1.0 + 0.6 * (r(H, W) - 0.3)), d)                  # outliers: depth errors over tau
        d[r(H, W) < 0.1] = 0
        depths.append(d)
        yaw = 0.03 * k + 0.01 * float(r(1)) - 0.02
        c, s = np.cos(yaw), np.sin(yaw)
        t = [0.35 * k + 0.05 * float(r(1)), 0.03 * float(r(1)), 0.04 * float(r(1))]
        poses.append(torch.tensor([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]], [0, 0, 0, 1]], dtype=torch.float64))
        fx, fy = 0.8 * W + float(r(1)), 0.8 * W + 1.0 + float(r(1))
        intr.append(torch.tensor([[fx, 0, W / 2 + float(r(1)) - 0.5], [0, fy, H / 2 + float(r(1)) - 0.5], [0, 0, 1]], dtype=torch.float64))
    f = lambda x: torch.stack(x).to(torch.float32)
    return dict(images=f(images), depths=f(depths), poses=f(poses), intr=f(intr))


def cast(S, dt):
    return {k: v.to(dt) for k, v in S.items()}


@functools.lru_cache(maxsize=None)
def scene(name):
    H, W, cam, it, conf_num, seed = SCENES[name]
    return make_scene(H, W, len(cam), seed)


@functools.lru_cache(maxsize=None)
def yard(name, modes):
    """-> (float64 maps, fp32 maps, {mode: d_mode}, diagnostics of the float64 passes); computed once and shared"""
    H, W, cam, it, conf_num, seed = SCENES[name]
    m64, diag = ref_precompute(cast(scene(name), torch.float64), cam, it, conf_num, modes, TAU)
    m32, _ = ref_precompute(scene(name), cam, it, conf_num, modes, TAU)
    d = {m: max(float((a[m].double() - b[m]).abs().max()) for a, b in zip(m32, m64)) for m in modes}
    return m64, m32, d, diag


def bound(d_mode):
    return max(4 * d_mode, 16 * EPS)


def check_precondition(diag, n_passes):
    assert len(diag) == n_passes
    for d in diag:
        assert d["tie"] > TIE and d["tau_gap"] > TAU_GAP, d
        assert d["n_in_view"] > 0 and all(v > 0 for v in d["range"].values()), d               # no empty pass, emax > emin


def intr4(K):
    return torch.stack([K[:, 0, 2], K[:, 1, 2], K[:, 0, 0], K[:, 1, 1]], -1).contiguous()


def modes_of(bits):
    return tuple(m for k, m in enumerate(ALL_MODES) if bits >> k & 1)


# ---- without a GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_passes", [("main", 6), ("tiles", 4)])
def test_scene_precondition(name, n_passes):
    m64, m32, d, diag = yard(name, ALL_MODES)
    check_precondition(diag, n_passes)
    H, W = SCENES[name][:2]
    print(f"{name}: d_mode = {d}, min tie distance {min(x['tie'] for x in diag):.2e} px, in view {[x['n_in_view'] for x in diag]} of {H * W}")
    assert any(x["n_in_view"] < H * W for x in diag)                                           # pixels out of view
    if name == "main":
        assert all(float(v.abs().max()) == 0 for v in m64[3].values())                         # the image without neighbours
        # depth-masked pixels exist, and the last-pass quirk shows: a pixel zeroed in rgb that the run without depth does not zero
        m_rgb, _, _, _ = yard(name, ("rgb",))
        assert any(bool(((a["rgb"] == 0) & (b["rgb"] != 0)).any()) for a, b in zip(m64[:3], m_rgb[:3]))
        assert [ref_select(SCENES[name][3], SCENES[name][2], i, 2) for i in range(4)] == [[1, 2], [2, 0], [1, 0], []]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not present")
def test_restatement_is_the_reference():
    for mod in ("turtle", "cv2", "imageio", "lpips", "kornia", "pyquaternion", "matplotlib", "matplotlib.pyplot", "nuscenes", "open3d", "skimage",
                "tqdm", "torchvision", "torchvision.models", "torchvision.transforms", "scipy.spatial.transform", "seaborn"):
        if mod not in sys.modules:
            try:
                __import__(mod)
            except Exception:
                class _Stub(types.ModuleType):          # plotting / dataset packages the confidence maps never call
                    __path__ = []

                    def __getattr__(self, k):
                        if k.startswith("__"):
                            raise AttributeError(k)
                        return type(k, (), {})
                sys.modules[mod] = _Stub(mod)
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    sys.path.insert(0, REF)
    try:
        import model.confidence as rc
        name = "main"
        H, W, cam, it, conf_num, seed = SCENES[name]
        S = scene(name)
        args = types.SimpleNamespace(conf_num=conf_num, flow=False)
        with torch.no_grad():
            got = rc.Confidence(list(ALL_MODES), "cpu", len(cam), vgg_loss=False, tau=TAU).precompute_conf_map(
                args, np.asarray(cam), S["images"], S["depths"], S["poses"], S["intr"], np.asarray(it))
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k not in saved_mods and k.split(".")[0] in ("model", "utils")]:
            del sys.modules[k]                          # the reference's top-level packages leave the process again
    m64, m32, d, diag = yard(name, ALL_MODES)
    assert len(got) == len(it)
    for p in range(len(it)):
        assert list(got[p].keys()) == list(ALL_MODES)
        for m in ALL_MODES:
            assert got[p][m].dtype == torch.float32 and tuple(got[p][m].shape) == (H * W,)
            dist = float((got[p][m].double() - m64[p][m]).abs().max())
            same = torch.equal(got[p][m], m32[p][m])
            print(f"position {p} {m}: reference fp32 vs float64 restatement {dist:.3e} (d_mode {d[m]:.3e}), bit-equal to the fp32 restatement: {same}")
            # the fp32 restatement is the reference's arithmetic: the reference may differ from float64 by that arithmetic's noise only
            assert dist <= 2 * d[m] + 4 * EPS, (p, m, dist, d[m])
            assert torch.equal(got[p][m] == 0, m64[p][m] == 0)                                 # no pixel flips its mask


def _abi_args():
    nb = (ctypes.c_int * 2)(1, 2)
    fake = 0x1000                                       # never dereferenced: every case below is refused before any launch
    return dict(images=fake, images_u8=0, depths=fake, poses=fake, intrinsics=fake, N=4, H=24, W=40, base=0, neighbours=nb, n_neighbours=2,
                modes=7, tau=0.2, ws=fake, ws_bytes=ops.reproj_conf_ws(24, 40), out_rgb=fake, out_ssim=fake, out_depth=fake, stream=None), nb


BAD_ARGS = [dict(images=None), dict(depths=None), dict(poses=None), dict(intrinsics=None), dict(N=0), dict(H=0), dict(W=0), dict(base=-1),
            dict(base=4), dict(neighbours=(ctypes.c_int * 2)(1, 4)), dict(neighbours=(ctypes.c_int * 2)(-1, 1)), dict(n_neighbours=-1),
            dict(neighbours=None), dict(modes=0), dict(modes=8), dict(out_rgb=None), dict(out_ssim=None), dict(out_depth=None),
            dict(ws=None), dict(ws_bytes="short"), dict(tau=float("nan")),
            dict(tau=float("inf"))]


@pytest.mark.parametrize("case", range(len(BAD_ARGS)))
def test_bad_arguments_are_refused_before_any_launch(case):
    a, keep = _abi_args()
    a.update(BAD_ARGS[case])
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = ops.reproj_conf_ws(a["H"], a["W"]) - 1
    sig = _lib.parse_header()["snerf_reproj_conf"]
    assert [n for _, n in sig] == list(a)
    assert _lib.load().snerf_reproj_conf(*[a[n] for _, n in sig]) == 1


def test_workspace_query():
    sizes = [ops.reproj_conf_ws(h, w) for h, w in ((1, 1), (11, 11), (24, 40), (45, 70), (900, 1600))]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes[1:])) == 4
    assert _lib.RESTYPE["snerf_reproj_conf_ws"] is ctypes.c_long


def test_select_conf_neighbours_is_the_reference_order():
    sel = confidence.select_conf_neighbours
    cases = [((0, 1, 2, 3), (0, 0, 0, 1), 2),           # camera change, both ends, conf_num = 2
             ((0, 1, 2, 3, 4, 5), (0, 0, 0, 1, 1, 1), 1),
             ((4, 2, 0, 5, 1, 3), (0, 1, 0, 1, 0, 0), 2),   # i_train not sorted by position: positions decide, images name the camera
             ((2, 0, 1), (0, 0, 0), 3)]                 # conf_num past both ends
    for it, cam, k in cases:
        for p, img in enumerate(it):
            assert sel(it, cam, p, k) == ref_select(it, np.asarray(cam), img, k), (it, cam, p, k)
    assert [sel((0, 1, 2, 3), (0, 0, 0, 1), p, 2) for p in range(4)] == [[1, 2], [2, 0], [1, 0], []]
    # position 2 holds image 0 (camera 0): +1 is image 5, -1 image 2, +2 image 1 (camera 1: left out), -2 image 4
    assert sel((4, 2, 0, 5, 1, 3), (0, 1, 0, 1, 0, 0), 2, 2) == [5, 2, 4]
    assert sel(np.asarray([0, 1, 2]), torch.tensor([0, 0, 0]), 1, 1) == [2, 0]


def test_vgg_and_flow_are_refused_with_a_way_out():
    args = types.SimpleNamespace(conf_num=1, flow=False, tau=0.2)
    with pytest.raises(NotImplementedError, match="ConfidenceMaps takes any mode names"):
        confidence.precompute_conf_map(args, [0], None, None, None, None, [0], modes=["rgb", "vgg"])
    with pytest.raises(NotImplementedError, match="ConfidenceMaps takes any mode names"):
        confidence.precompute_conf_map(types.SimpleNamespace(conf_num=1, flow=True), [0], None, None, None, None, [0], modes=["rgb"])
    net = confidence.Confidence(["rgb", "depth"], 3)
    with pytest.raises(NotImplementedError, match="flow"):
        net.precompute_conf_map(args, [0], None, None, None, None, [0], flow=[None])
    with pytest.raises(NotImplementedError, match="VGG"):
        confidence.Confidence(["rgb", "vgg"], 3).precompute_conf_map(args, [0], None, None, None, None, [0])


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------
def device_scene(name):
    S = scene(name)
    return S["images"].cuda().contiguous(), S["depths"].cuda().contiguous(), S["poses"][:, :3, :4].cuda().contiguous(), intr4(S["intr"]).cuda()


def device_maps(name, modes, images=None):
    """[P][M,H,W] on the device through ops.reproj_conf and the reference's neighbour order"""
    H, W, cam, it, conf_num, seed = SCENES[name]
    img, dep, P, K = device_scene(name)
    img = img if images is None else images
    return [ops.reproj_conf(img, dep, P, K, b, confidence.select_conf_neighbours(it, cam, p, conf_num), modes, TAU) for p, b in enumerate(it)]


def compare(name, modes):
    H, W = SCENES[name][:2]
    m64, m32, d, diag = yard(name, modes)
    got = device_maps(name, modes)
    worst = {m: 0.0 for m in modes}
    for p in range(len(got)):
        g = got[p].cpu().double().reshape(len(modes), H * W)
        for k, m in enumerate(modes):
            worst[m] = max(worst[m], float((g[k] - m64[p][m]).abs().max()))
    for m in modes:
        print(f"{name} {'+'.join(modes)} {m}: d_mode {d[m]:.3e}, bound {bound(d[m]):.3e}, kernel vs float64 {worst[m]:.3e}")
    for m in modes:
        assert worst[m] <= bound(d[m]), (m, worst[m], d[m])
    return worst


@gpu
@pytest.mark.parametrize("bits", range(1, 8))
def test_every_mode_subset_against_the_restatement(bits):
    compare("main", modes_of(bits))


@gpu
def test_second_shape_spans_tiles_and_borders():
    check_precondition(yard("tiles", ALL_MODES)[3], 4)
    compare("tiles", ALL_MODES)


@gpu
def test_uint8_images_equal_their_fp32_decode_bit_for_bit():
    H, W, cam, it, conf_num, seed = SCENES["main"]
    u8 = torch.randint(0, 256, (len(cam), H, W, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    f32 = torch.tensor(u8.numpy().astype(np.float64) / 255.0, dtype=torch.float64).to(torch.float32)
    a, b = device_maps("main", ALL_MODES, u8.cuda()), device_maps("main", ALL_MODES, f32.cuda())
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert float(a[0].abs().max()) > 0


@gpu
def test_two_calls_give_identical_bits():
    a, b = device_maps("main", ALL_MODES), device_maps("main", ALL_MODES)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def away_scene():
    """the main scene plus image 4, posed to look away from everything the others see: turned by a quarter turn and lifted far up, so
    no pixel of any base (pixels of depth 0 included) lands in its view"""
    S = {k: v.clone() for k, v in scene("main").items()}
    away = torch.tensor([[0., 0, 1, 0.3], [0, 1, 0, 500.], [-1, 0, 0, 0.1], [0, 0, 0, 1]])
    return dict(images=torch.cat([S["images"], S["images"][:1]]), depths=torch.cat([S["depths"], S["depths"][:1]]),
                poses=torch.cat([S["poses"], away[None]]), intr=torch.cat([S["intr"], S["intr"][:1]]))


@gpu
def test_an_empty_last_pass_changes_nothing():
    S = away_scene()
    for base in (0, 1):
        assert not bool(ref_warping(cast(S, torch.float64), base, 4)[3].any())                 # nothing in view, in float64
    img, dep, P, K = S["images"].cuda(), S["depths"].cuda(), S["poses"][:, :3, :4].contiguous().cuda(), intr4(S["intr"]).cuda()
    for base, nb in ((0, [1, 2]), (1, [2, 0])):
        a = ops.reproj_conf(img, dep, P, K, base, nb, ALL_MODES, TAU)
        b = ops.reproj_conf(img, dep, P, K, base, nb + [4], ALL_MODES, TAU)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        c = ops.reproj_conf(img, dep, P, K, base, [4], ALL_MODES, TAU)                         # only empty passes: zeros
        assert float(c.abs().max()) == 0


@gpu
def test_no_neighbours_gives_zeros():
    img, dep, P, K = device_scene("main")
    out = torch.full((3, 24, 40), 7.0, device="cuda")
    ops.reproj_conf(img, dep, P, K, 3, [], ALL_MODES, TAU, out=out)
    assert float(out.abs().max()) == 0


@gpu
def test_captured_in_a_graph_and_replayed():
    img, dep, P, K = device_scene("main")
    H, W = SCENES["main"][:2]
    eager = ops.reproj_conf(img, dep, P, K, 1, [2, 0], ALL_MODES, TAU)
    out = torch.zeros(3, H, W, device="cuda")
    ws = torch.empty(ops.reproj_conf_ws(H, W), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.reproj_conf(img, dep, P, K, 1, [2, 0], ALL_MODES, TAU, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.reproj_conf(img, dep, P, K, 1, [2, 0], ALL_MODES, TAU, out=out, ws=ws)
    out.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), eager.view(torch.int32))


def _batcher(name):
    from snerf_amd.sample_utils import ImageRayBatcher
    H, W, cam, it, conf_num, seed = SCENES[name]
    S = scene(name)
    args = types.SimpleNamespace(no_ndc=True, N_rgb=64, conf_num=conf_num, flow=False, tau=TAU, no_reproj=False, no_geometry=False, vgg_loss=False)
    b = ImageRayBatcher(args, S["images"], S["depths"], S["poses"], S["intr"], np.asarray(it), 2.0, 20.0, camera_index=np.asarray(cam), device="cuda")
    return args, b


@gpu
def test_end_to_end_through_the_batcher_and_the_learned_mix():
    H, W, cam, it, conf_num, seed = SCENES["main"]
    m64, m32, d, diag = yard("main", ALL_MODES)
    args, b = _batcher("main")
    net = confidence.Confidence(list(ALL_MODES), len(cam), tau=TAU).cuda()
    with torch.no_grad():
        net.lambdas.copy_(torch.rand(3, len(cam), generator=torch.Generator().manual_seed(2)) * 4 - 2)
    maps = net.precompute_conf_map(args, cam, None, None, None, None, it, batcher=b)
    assert all(v.is_cuda for dct in maps for v in dct.values())
    cm = confidence.ConfidenceMaps(maps, it, len(cam), H, W)                                    # no device argument: the maps stay where they are
    assert cm.maps.is_cuda and tuple(cm.maps.shape) == (3, len(it), H, W) and cm.modes == list(ALL_MODES) and cm.slot_of_image.is_cuda
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sel = torch.stack([ys.reshape(-1), xs.reshape(-1)], -1)
    for img_i in it:
        # a convex mix of the maps: their bounds mix with the same weights; plus the mix's own roundings on values <= 1 (per mode the
        # weight, a product and an add; the weights' sum; the division)
        w = torch.sigmoid(net.lambdas.detach().cpu().double()[:, img_i])
        tol = float((w * torch.tensor([bound(d[m]) for m in ALL_MODES], dtype=torch.float64)).sum() / w.sum()) + (3 * 3 + 4) * EPS
        got = confidence.calc_final_confidence(net, cm, sel.cuda(), img_i).detach().cpu().double()
        want = ref_final_confidence(net.lambdas.detach().cpu(), ALL_MODES, m64, it, img_i, sel, H, W)
        dist = float((got - want).abs().max())
        print(f"image {img_i}: mixed confidence vs float64 {dist:.3e} (bound {tol:.3e})")
        assert dist <= tol


@gpu
def test_the_returned_list_has_the_reference_structure():
    H, W, cam, it, conf_num, seed = SCENES["main"]
    S = scene("main")
    args = types.SimpleNamespace(conf_num=conf_num, flow=False, tau=TAU)
    for poses, intr in ((S["poses"], S["intr"]), (S["poses"][:, :3, :4], intr4(S["intr"]))):     # [N,4,4] + 3x3, [N,3,4] + [N,4]
        maps = confidence.precompute_conf_map(args, cam, S["images"], S["depths"], poses, intr, it, modes=["depth", "rgb"])
        assert isinstance(maps, list) and len(maps) == len(it)
        for dct in maps:
            assert list(dct.keys()) == ["depth", "rgb"]
            assert all(v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (H * W,) for v in dct.values())
    m64 = yard("main", ("depth", "rgb"))
    for p in range(len(it)):
        for m in ("depth", "rgb"):
            assert float((maps[p][m].cpu().double() - m64[0][p][m]).abs().max()) <= bound(m64[2][m])
