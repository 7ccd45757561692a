"""Learned camera poses (pose_refine = True of both shipped S-NeRF configs): the per-image table of s-nerf/model/poses.py:6-36 with the
axis-angle map of utils/lie_group_helper.py:47-81.

`LearnPose` keeps the reference's parameter names (`r`, `t`, `init_c2w`), so a `pose/NNNNNN.tar` `model_param` dict loads with
`load_state_dict`, and its `forward` in torch ops: evaluation and rendering at the refined poses (`c2w @ init_c2w[cam_id]`), and callers
who keep their own training loop (sample_utils.apply_pose_transform + MipTrainer.step(ray_grads=True)).  Training on the device goes
through `MipTrainer(pose_net=...)`: the table row is applied to the batch by `snerf_pose_apply` and the ray gradients are reduced to
the row's gradient by `snerf_pose_grad`; `pose_grad_chain` below is that kernel's host model in float64.

That is the training-time route (sample_utils.py:421-435, transform_only=True): finished rays are moved, o + t and R d.  The test-time
route (s-nerf/eval.py:77-114, --test_refine_iter) fits the test cameras against the trained network, which is held fixed, and generates
its rays from make_c2w(r, t) @ init_c2w[img]: the camera centre turns with the rotation, o' = R o + t, d' = R d -- the delta applied to
the rays of the INITIAL pose, which is what `snerf_pose_compose_apply` does; `snerf_pose_compose_grad` adds the term sum g_o o^T to the
rotation's gradient (`pose_sums(..., origins=o)`).  `MipTrainer(pose_net=..., freeze_model=True, pose_compose=True)` is that loop on the
device: data gradients only, no weight gradient, no arena Adam; afterwards `pose_net(i)` is the refined pose of image i.

Path C's pose refinement (s-nerfpp/zipnerf/train.py:177-213, 338-344; internal/posenet_v2.py) moves every ray by the row of its own
camera -- a batch mixes cameras -- turns base_x / base_y as well, scales the translation by `t_ratio` and trains the table with plain
SGD.  `LearnPoseV2` is that module in torch ops (its `posenet_ckpt_*` state_dict loads); `zipnerf.apply_pose` applies its output to a
batch; on the device `ZipTrainer(pose_net=...)` runs `snerf_pose_table`, `snerf_pose_rays_apply` and `snerf_pose_rays_grad`, whose
float64 host model is `pose_rays_sums` + `pose_grad_chain`."""
import torch
import torch.nn as nn


def skew(r):
    """[3] -> the [3,3] cross-product matrix K with K x = r x x"""
    z = torch.zeros((), dtype=r.dtype, device=r.device)
    return torch.stack([torch.stack([z, -r[2], r[1]]), torch.stack([r[2], z, -r[0]]), torch.stack([-r[1], r[0], z])])


def rotation(r):
    """axis-angle [3] -> rotation [3,3], lie_group_helper.Exp as written: I + (sin th / th) K + ((1 - cos th) / th^2) K K with
    th = |r| + 1e-15 (no small-angle branch: at r = 0 the matrix is I because K is 0)"""
    K = skew(r)
    th = r.norm() + 1e-15
    return torch.eye(3, dtype=r.dtype, device=r.device) + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / th ** 2) * (K @ K)


class LearnPose(nn.Module):
    def __init__(self, num_cams, learn_R, learn_t, init_c2w=None):
        """num_cams rows of axis-angle `r` and translation `t` (zeros: the identity), trained when learn_R / learn_t;
        init_c2w [num_cams,4,4] (optional, never trained): the poses the learned transforms are deltas to"""
        super().__init__()
        self.num_cams = int(num_cams)
        self.init_c2w = None
        if init_c2w is not None:
            self.init_c2w = nn.Parameter(torch.as_tensor(init_c2w).detach().clone(), requires_grad=False)
        self.r = nn.Parameter(torch.zeros(self.num_cams, 3, dtype=torch.float32), requires_grad=bool(learn_R))
        self.t = nn.Parameter(torch.zeros(self.num_cams, 3, dtype=torch.float32), requires_grad=bool(learn_t))

    def forward(self, cam_id, transform_only=False):
        """-> [4,4]: the learned transform [R(r) | t] of image cam_id, or (transform_only=False, with init_c2w) that times init_c2w[cam_id]"""
        r, t = self.r[cam_id], self.t[cam_id]
        top = torch.cat([rotation(r), t[:, None]], dim=1)
        c2w = torch.cat([top, torch.tensor([[0, 0, 0, 1]], dtype=top.dtype, device=top.device)], dim=0)
        if not transform_only and self.init_c2w is not None:
            c2w = c2w @ self.init_c2w[cam_id]
        return c2w


def rotations(r):
    """`rotation` for a whole table: axis-angle [N,3] -> [N,3,3], posenet_v2.Exp as written"""
    z = torch.zeros_like(r[:, 0])
    K = torch.stack([torch.stack([z, -r[:, 2], r[:, 1]], 1), torch.stack([r[:, 2], z, -r[:, 0]], 1), torch.stack([-r[:, 1], r[:, 0], z], 1)], 1)
    th = r.norm(dim=-1)[:, None, None] + 1e-15
    return torch.eye(3, dtype=r.dtype, device=r.device)[None] + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / th ** 2) * (K @ K)


class LearnPoseV2(nn.Module):
    def __init__(self, num_cams, learn_R=True, learn_t=True, init_c2w=None, t_ratio=1):
        """posenet_v2.LearnPose: num_cams rows of axis-angle `r` and translation `t` (zeros: the identity), the translation applied as
        t * t_ratio (configs.py:145: 0.25); init_c2w [num_cams,4,4] (optional, never trained)"""
        super().__init__()
        self.num_cams, self.t_ratio = int(num_cams), t_ratio
        self.init_c2w = None
        if init_c2w is not None:
            self.init_c2w = nn.Parameter(torch.as_tensor(init_c2w).detach().clone(), requires_grad=False)
        self.r = nn.Parameter(torch.zeros(self.num_cams, 3, dtype=torch.float32), requires_grad=bool(learn_R))
        self.t = nn.Parameter(torch.zeros(self.num_cams, 3, dtype=torch.float32), requires_grad=bool(learn_t))

    def forward(self, cam_id, transform_only=False, one_img=False):
        """cam_id [B] (integer) -> [B,4,4]: the learned transforms [R(r) | t * t_ratio] of those rows, or (transform_only=False, with
        init_c2w) those times init_c2w[cam_id]; one_img: the bare transform of row cam_id[0] alone, [1,4,4]"""
        cam_id = torch.as_tensor(cam_id, device=self.r.device).reshape(-1).long()
        if one_img:
            cam_id = cam_id[:1]
        top = torch.cat([rotations(self.r), (self.t * self.t_ratio)[:, :, None]], dim=2)
        c2w = torch.cat([top, torch.zeros_like(top[:, :1])], dim=1)
        c2w[:, 3, 3] = 1.0
        c2w = c2w[cam_id]
        if not one_img and not transform_only and self.init_c2w is not None:
            c2w = c2w @ self.init_c2w[cam_id]
        return c2w


def pose_rays_sums(cam, n_cams, g_o, g_d, g_v, g_bx, g_by, directions, viewdirs, base_x, base_y, t_ratio=1.0):
    """Host model of snerf_pose_rays_grad's reduction, float64: cam [n] (each ray's table row, truncated toward zero; rows outside
    [0, n_cams) take no part) -> (G [n_cams,3,3], g_t [n_cams,3], count [n_cams]) with G_c = sum over the rays of camera c of
    g_d d^T + g_v v^T + g_bx bx^T + g_by by^T (the UNmoved rays) and g_t,c = t_ratio * sum g_o.  `pose_grad_chain(r[c], G[c])` is
    then row c of the rotation's gradient."""
    f = lambda x: torch.as_tensor(x).detach().cpu().to(torch.float64)
    c = torch.trunc(f(cam).reshape(-1))
    ok = (c >= 0) & (c < n_cams)                                                        # (a NaN index compares false)
    idx = c[ok].long()
    outer = sum(f(g)[ok][:, :, None] * f(x)[ok][:, None, :] for g, x in ((g_d, directions), (g_v, viewdirs), (g_bx, base_x), (g_by, base_y)))
    G = torch.zeros(n_cams, 3, 3, dtype=torch.float64).index_add_(0, idx, outer)
    g_t = torch.zeros(n_cams, 3, dtype=torch.float64)
    if g_o is not None:
        g_t.index_add_(0, idx, f(g_o)[ok] * float(t_ratio))
    count = torch.zeros(n_cams, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
    return G, g_t, count


def pose_grad_chain(r, G):
    """Host model of snerf_pose_grad's chain, float64: r [3] (one table row), G [3,3] = d loss / d R -> d loss / d r [3], the derivative
    of `rotation` as autograd takes it:
        dL/dr_k = A <G, E_k> + B <G, E_k K + K E_k> + (A' <G, K> + B' <G, K K>) r_k / |r|,     E_k = dK/dr_k,
        A = sin th / th,  B = (1 - cos th) / th^2,  A' = (th cos th - sin th) / th^2,  B' = (th sin th - 2 (1 - cos th)) / th^3,
    the last term dropped at |r| = 0, where torch's norm has the subgradient 0 (and where training starts)."""
    r = torch.as_tensor(r, dtype=torch.float64).reshape(3)
    G = torch.as_tensor(G, dtype=torch.float64).reshape(3, 3)
    K = skew(r)
    nr = r.norm()
    th = nr + 1e-15
    sn, cs = torch.sin(th), torch.cos(th)
    A, B = sn / th, (1 - cs) / th ** 2
    dA, dB = (th * cs - sn) / th ** 2, (th * sn - 2 * (1 - cs)) / th ** 3
    out = torch.zeros(3, dtype=torch.float64)
    radial = dA * (G * K).sum() + dB * (G * (K @ K)).sum()
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[k] = 1.0
        E = skew(e)
        out[k] = A * (G * E).sum() + B * (G * (E @ K + K @ E)).sum()
        if float(nr) > 0:
            out[k] = out[k] + radial * r[k] / nr
    return out


def pose_sums(g_o, g_d, g_v, directions, viewdirs, origins=None):
    """the twelve float64 sums snerf_pose_grad forms over a batch -> (G [3,3], g_t [3]); with `origins` (the untransformed ones) those of
    snerf_pose_compose_grad: the rotation reaches the origins too, so G gains sum g_o o^T"""
    f = lambda x: torch.as_tensor(x).detach().cpu().to(torch.float64)
    G = f(g_d).T @ f(directions) + f(g_v).T @ f(viewdirs)
    if origins is not None:
        G = G + f(g_o).T @ f(origins)
    return G, f(g_o).sum(0)
