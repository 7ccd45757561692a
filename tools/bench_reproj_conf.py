#!/usr/bin/env python3
"""Reprojection confidence maps (configs: depth_conf = True, precompute_conf = True) at the shipped nuScenes shape on one MI355X:
900 x 1600 uint8 images, 6 cameras x --frames frames (camera-major), conf_num = 1, modes rgb + ssim + depth.

    device  confidence.precompute_conf_map(batcher-resident tensors): snerf_reproj_conf, one warp / ssim / finish / accumulate launch per
            (base, neighbour) pass; device events around the whole call after --warmup calls, --rounds times, median; ms per pass =
            that over the number of passes
    eager   the same computation as a user would otherwise run it: the reference's get_reproj_conf restated in torch (grid_sample,
            depthwise conv2d, boolean-mask indexing) in fp32 on the same GPU, timed per pass the same way over one camera's passes

The two alternate within a round.  Also reported: ms for a 240-image training set (6 cameras x 40 frames: 6 x 78 passes), the largest
difference between the two routes' maps, and the pass's compulsory HBM traffic (both uint8 images and both depth maps read once, the
three maps written once) over its time as a fraction of the 8 TB/s peak.  --kernels-only runs just the device route a few times, for a
kernel trace taken in a run of its own (each kernel's share of the time).  Prints one JSON line; --out also writes it to a text file."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

MODES = ["rgb", "ssim", "depth"]
HBM_PEAK = 8.0e12


def scene(n_cam, frames, H, W, dev):
    """procedural stand-in for a nuScenes clip: textured uint8 images, depths of 5-60 m with 10 % holes, cameras that drive forward"""
    g = torch.Generator(device=dev).manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    images, depths, poses, K = [], [], [], []
    for c in range(n_cam):
        for f in range(frames):
            tex = torch.stack([0.5 + 0.25 * torch.sin(0.021 * (xs + 9 * f) + ch + c) * torch.cos(0.017 * ys + 0.5 * ch) +
                               0.1 * torch.sin(0.13 * xs + 0.11 * ys + ch) for ch in range(3)], -1)
            tex = (tex + 0.05 * (torch.rand(H, W, 3, generator=g, device=dev) - 0.5)).clamp(0, 1)
            images.append((tex * 255).round().to(torch.uint8))
            d = 30 + 25 * torch.sin(0.002 * xs + 0.3 * c) * torch.cos(0.003 * ys) + torch.rand(H, W, generator=g, device=dev)
            d[torch.rand(H, W, generator=g, device=dev) < 0.1] = 0
            depths.append(d)
            yaw = 1.047 * c + 0.004 * f
            cs, sn = np.cos(yaw), np.sin(yaw)
            poses.append(torch.tensor([[cs, 0, sn, 0.1 * f * sn], [0, 1, 0, 0.0], [-sn, 0, cs, -0.5 * f * cs]], dtype=torch.float32))
            K.append(torch.tensor([W / 2 + 3.0, H / 2 - 2.0, 1266.0, 1268.0], dtype=torch.float32))
    return torch.stack(images), torch.stack(depths), torch.stack(poses).to(dev), torch.stack(K).to(dev)


# ---- the eager form: get_reproj_conf (s-nerf/model/loss.py:271-327) as torch ops on the device ----------------------------------------
def eager_window(dev):
    g = torch.Tensor([np.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w1 = (g / g.sum()).unsqueeze(1)
    return w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0).expand(3, 1, 11, 11).contiguous().to(dev)


def eager_pass(img, dep, pose4, K, base, tgt, tau, window):
    H, W = img.shape[1:3]
    proj = torch.flip(torch.nonzero(torch.ones((H, W), device=img.device)), [1])
    focal, tfocal = (K[base, 2] + K[base, 3]) / 2, (K[tgt, 2] + K[tgt, 3]) / 2
    i, j = (proj[:, 0] - K[base, 0]) / focal, -(proj[:, 1] - K[base, 1]) / focal
    dirs = torch.stack([i, j, -torch.ones_like(i)], -1).permute(1, 0) * dep[base].reshape(-1)
    dirs = F.pad(dirs.permute(1, 0), (0, 1), "constant", 1).float()
    cam = (torch.inverse(pose4[tgt]) @ (pose4[base] @ dirs.T))[:3].T
    depth = cam[:, 2].abs()
    uv = torch.stack([cam[:, 0] / depth * tfocal + K[tgt, 0], -(cam[:, 1] / depth * tfocal) + K[tgt, 1]], -1)
    xr, yr = uv[:, 1].round(), uv[:, 0].round()
    mask = (xr >= 0) & (xr < H) & (yr >= 0) & (yr < W)
    grid = torch.stack([uv[mask][:, 0] / ((W - 1) // 2) - 1, uv[mask][:, 1] / ((H - 1) // 2) - 1], -1)
    rgb = F.grid_sample(img[tgt].unsqueeze(0).permute(0, 3, 1, 2), grid[None, ...].unsqueeze(2), align_corners=False).squeeze(3).squeeze(0).T
    fake = torch.zeros_like(img[base])
    co = proj[mask]
    fake[co[:, 1], co[:, 0]] = rgb
    m2 = mask.reshape(H, W)
    base_ = img[base].clone()
    base_[~m2] = 0
    err = {"rgb": (base_ - fake).abs().mean(2)[m2]}
    a, b = base_[None].permute(0, 3, 1, 2), fake[None].permute(0, 3, 1, 2)
    conv = lambda x: F.conv2d(x, window, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1.pow(2), conv(b * b) - mu2.pow(2), conv(a * b) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 1e-4) * (2.0 * s12 + 9e-4)) / ((mu1.pow(2) + mu2.pow(2) + 1e-4) * (s1 + s2 + 9e-4))
    err["ssim"] = (1 - ssim.mean(1))[0][m2]
    td = dep[tgt][xr[mask].long(), yr[mask].long()]
    err["depth"] = (depth[mask] - td).abs() / torch.max(td, torch.tensor(1e-10, device=img.device))
    dmask = err["depth"] > tau
    err["depth"] = torch.clamp(err["depth"], max=tau)
    conf = {}
    for m in MODES:
        c = err[m].max() - err[m]
        conf[m] = c / c.max()
    return conf, mask, dmask


def eager_maps(img, dep, pose4, K, base, neighbours, tau, window):
    H, W = img.shape[1:3]
    confs = {m: torch.zeros(H * W, device=img.device) for m in MODES}
    cnt = torch.zeros(H * W, device=img.device)
    for tgt in neighbours:
        conf, mask, dmask = eager_pass(img, dep, pose4, K, base, tgt, tau, window)
        for m in MODES:
            confs[m][mask] += conf[m]
        cnt[mask] += 1
    cnt[cnt == 0] = 1
    for m in MODES:
        confs[m] /= cnt
        t = confs[m][mask]
        t[dmask] = 0.
        confs[m][mask] = t
    return confs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--height", type=int, default=900)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from snerf_amd import confidence
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n_cam, fr, H, W = 6, args.frames, args.height, args.width
    images, depths, poses, K = scene(n_cam, fr, H, W, dev)
    N = n_cam * fr
    cam_index, i_train = [k // fr for k in range(N)], list(range(N))
    tau = 0.2
    cargs = types.SimpleNamespace(conf_num=1, flow=False, tau=tau)
    resident = types.SimpleNamespace(images=images, depths=depths, poses=poses, intrinsics=K)      # what an ImageRayBatcher holds
    passes = sum(len(confidence.select_conf_neighbours(i_train, cam_index, p, 1)) for p in range(N))
    device_route = lambda: confidence.precompute_conf_map(cargs, cam_index, None, None, None, None, i_train, modes=MODES, batcher=resident)
    for _ in range(args.warmup):
        maps = device_route()
    torch.cuda.synchronize()
    if args.kernels_only:
        for _ in range(3):
            device_route()
        torch.cuda.synchronize()
        print(json.dumps({"kernels_only": True, "passes_per_call": passes, "calls": 3 + args.warmup}))
        return

    img_f = images[:fr].float() / 255.0                                                            # one camera's frames for the eager route
    pose4 = torch.cat([poses[:fr], torch.tensor([0., 0, 0, 1], device=dev).expand(fr, 1, 4)], 1)
    window = eager_window(dev)
    e_sel = [confidence.select_conf_neighbours(i_train[:fr], cam_index[:fr], p, 1) for p in range(fr)]
    e_passes = sum(len(s) for s in e_sel)
    eager_route = lambda: [eager_maps(img_f, depths[:fr], pose4, K[:fr], p, e_sel[p], tau, window) for p in range(fr)]
    for _ in range(args.warmup):
        e_maps = eager_route()
    torch.cuda.synchronize()
    diff = {m: max(float((maps[p][m] - e_maps[p][m]).abs().max()) for p in range(fr)) for m in MODES}
    differing = {m: sum(int(((maps[p][m] - e_maps[p][m]).abs() > 1e-3).sum()) for p in range(fr)) for m in MODES}

    dev_ms, eag_ms = [], []
    for _ in range(args.rounds):
        dev_ms.append(timed(device_route) / passes)
        eag_ms.append(timed(eager_route) / e_passes)
    d, e = statistics.median(dev_ms), statistics.median(eag_ms)
    u8 = images.dtype == torch.uint8
    compulsory = H * W * ((6 if u8 else 24) + 8 + 12)
    res = {"shape": [N, H, W], "images": "uint8" if u8 else "fp32", "modes": MODES, "conf_num": 1, "passes_per_call": passes,
           "device_ms_per_pass": round(d, 4), "eager_ms_per_pass": round(e, 4), "eager_over_device": round(e / d, 2),
           "device_ms_240_images": round(d * 6 * 78, 1), "eager_ms_240_images": round(e * 6 * 78, 1),
           "device_ms_per_pass_rounds": [round(x, 4) for x in dev_ms], "eager_ms_per_pass_rounds": [round(x, 4) for x in eag_ms],
           "max_abs_diff_device_vs_eager_fp32": diff, "pixels_differing_by_more_than_1e-3": differing,
           "compulsory_bytes_per_pass": compulsory, "fraction_of_hbm_peak_on_compulsory_traffic": round(compulsory / (d * 1e-3) / HBM_PEAK, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_reproj_conf.py: reprojection confidence maps (rgb + ssim + depth, conf_num = 1), one MI355X, ms per (base, neighbour) pass;\n")
            f.write("# device = confidence.precompute_conf_map on resident tensors (snerf_reproj_conf), eager = the reference's get_reproj_conf as torch ops in\n")
            f.write("# fp32 on the same GPU; device events, the two alternate within a round, the summary holds the medians.\n")
            f.write(line + "\n")


if __name__ == "__main__":
    main()
