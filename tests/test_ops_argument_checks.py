"""The binding layer's argument checks: they raise _lib.SnerfArgumentError before anything reaches the library, with or without
`python -O`, and they change nothing about a valid call.

In every test `_lib.call` / `_lib.query` are stubs (`call` records, `query` returns a fixed size) and `_stream` returns 0, so nothing is
ever launched: what a broken checker lets through reaches the stub and fails an assertion here, never a kernel.

Without a GPU the valid arguments of a call are CPU tensors of a subclass that answers `is_cuda` with True; the argument under test is a
plain CPU tensor.  The `gpu` tests run the same table on real device tensors (a few hundred elements each).

A second table (`_tightened`) holds a minimal valid call for every wrapper with a tensor whose hand-written chain had forgotten the device
or the contiguity check: each such tensor is refused on the CPU and as a non-contiguous view, with and without a GPU.

Two wrappers of the table check no shape of their own (mip_composite_fwd, grid_encode_fwd: the library does), so they have no
wrong-shape case; a short workspace is a case only where the wrapper owns that check (reproj_conf, frame_metrics, mesh_prepare,
mesh_trace_pinhole) -- elsewhere the library refuses it with status 1, which tests/test_shadow.py and others pin."""
import ast
import ctypes
import importlib.machinery
import importlib.util
import os
import re

import pytest
import torch

import snerf_amd
from snerf_amd import _lib, foreground, ops

MODULES = ("ops", "foreground", "shadow", "meshtrace", "meshrender", "metrics")
QUERY = 256                                  # what the `query` stub answers: every workspace size of these tests
f32, bf16, i32, i64, u8, f64 = torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.float64


class _OnDevice(torch.Tensor):
    """a CPU tensor that claims to live on the device: the valid arguments of the tests that run without a GPU"""
    is_cuda = property(lambda self: True)


def _fake(t):
    return t.as_subclass(_OnDevice)


def _real(t):
    return t.cuda()


def _z(*shape, dt=f32):
    return torch.zeros(*shape, dtype=dt)


# ---- the table: one representative wrapper per family -> (module, function, kwargs, loose, wrong_shape, short_ws) --------------------------
# kwargs: a valid call, tensors made by `mk`; loose: tensor arguments the wrapper only asks to be on the device; wrong_shape: (argument,
# CPU tensor of a shape the wrapper refuses) or None; short_ws: the workspace argument whose size the wrapper checks, or None
def _cases(mk):
    n, S = 4, 3
    img = lambda *sh: mk(_z(*sh, dt=u8))
    rays = lambda: mk(_z(n, 3))
    return {
        "linear_fwd": ("ops", "linear_fwd", dict(A=mk(_z(4, 32, dt=bf16)), W=mk(_z(8, 32, dt=bf16)), bias=mk(_z(8)), Y=mk(_z(4, 8, dt=bf16)), K=32,
                                                 n_store=8, act=ops.ACT_MASK, dt=ops.BF16, aux=mk(_z(4, 8, dt=bf16)), colsum=mk(_z(8))),
                       {"bias", "colsum"}, ("Y", _z(5, 8, dt=bf16)), None),
        "linear_fwd_bits": ("ops", "linear_fwd", dict(A=mk(_z(4, 32, dt=bf16)), W=mk(_z(8, 32, dt=bf16)), bias=mk(_z(8)), Y=mk(_z(4, 8, dt=bf16)),
                                                      K=32, n_store=8, act=ops.ACT_RELU_BITS, dt=ops.BF16, aux=mk(_z(4, dt=i32))),
                            {"bias"}, ("A", _z(4, 16, dt=bf16)), None),
        "linear_wgrad": ("ops", "linear_wgrad", dict(dZ=mk(_z(8, 16, dt=bf16)), X=mk(_z(8, 32, dt=bf16)), dW=mk(_z(16, 32)), n_valid=16, k_valid=32,
                                                     dt=ops.BF16), set(), ("X", _z(7, 32, dt=bf16)), None),
        "fmlp_proposal_fwd": ("ops", "fmlp_proposal_fwd", dict(E=mk(_z(4, 96, dt=bf16)), stream=mk(_z(64, dt=bf16)), bias=mk(_z(32)),
                                                               raw_density=mk(_z(4, 1))), set(), ("raw_density", _z(5, 1)), None),
        "mip_composite_fwd": ("ops", "mip_composite_fwd", dict(raw_rgb=mk(_z(n * S, 3)), raw_density=mk(_z(n * S, 1)), noise=mk(_z(n, S)),
                                                               s_vals=mk(_z(n, S + 1)), dirs=rays(), near=mk(_z(n, 1)), far=mk(_z(n, 1)), transform_idx=0,
                                                               white=False, rgb_padding=.001, density_bias=-1., row_index=mk(_z(n, S, dt=i32))),
                              {"raw_rgb", "raw_density", "row_index"}, None, None),
        "adam_step": ("ops", "adam_step", dict(p=mk(_z(32)), g=mk(_z(32)), m=mk(_z(32)), v=mk(_z(32)), lr=1e-3, b1=.9, b2=.999, eps=1e-8, step=1,
                                               clip_coef=mk(_z(2)), step_dev=mk(_z(1, dt=i32)), lr_dev=mk(_z(1)), dropped=mk(_z(1, dt=i64))),
                      set(), ("step_dev", _z(2, dt=i32)), None),
        "gather_pack": ("ops", "gather_pack", dict(flat=mk(_z(16)), idx=mk(_z(8, dt=i32)), dst=mk(_z(8, dt=bf16)), tiles=mk(_z(2, 4, dt=i32))),
                        set(), ("dst", _z(9, dt=bf16)), None),
        "grid_encode_fwd": ("ops", "grid_encode_fwd", dict(inputs=mk(_z(4, 3)), embeddings=mk(_z(16, 2)), offsets=mk(_z(3, dt=i32)), L=2, S=1., H=4,
                                                           gridtype=0, align_corners=False, interp=0), set(), None, None),
        "zip_encode_bwd": ("ops", "zip_encode_bwd", dict(tdist=mk(_z(2, 4)), origins=mk(_z(2, 3)), directions=mk(_z(2, 3)), radii=mk(_z(2, 1)),
                                                         base_x=mk(_z(2, 3)), base_y=mk(_z(2, 3)), deg_jitter=mk(_z(2, 3)), offsets=mk(_z(3, dt=i32)),
                                                         grid_sizes=mk(_z(2, dt=i32)), grad_feat=mk(_z(6, 8)), grad_table=mk(_z(16, 4)), L=2, C=4, n=2,
                                                         m=1, Sl=1., H=4, std_scale=.5, grad_table_bf16=mk(_z(16, 4, dt=bf16))),
                           {"tdist", "origins", "directions", "radii", "base_x", "base_y", "deg_jitter", "offsets", "grid_sizes", "grad_feat"},
                           ("grad_table_bf16", _z(15, 4, dt=bf16)), None),
        "smooth_loss": ("ops", "smooth_loss", dict(rgb=mk(_z(8, 3)), dist=mk(_z(8)), sky=mk(_z(8)), P=2, p=2, weight=.1, out=mk(_z(3)), total=mk(_z(1)),
                                                   g_dist=mk(_z(8)), accumulate=True, ws=mk(_z(16, dt=f64))), set(), ("dist", _z(7)), None),
        "pose_apply": ("ops", "pose_apply", dict(r=mk(_z(3, 3)), t=mk(_z(3, 3)), cam=mk(_z(1, dt=i64)), origins=rays(), directions=rays(), viewdirs=rays(),
                                                 pose_out=mk(_z(3, 4))), set(), ("directions", _z(5, 3)), None),
        "conf_apply": ("ops", "conf_apply", dict(maps=mk(_z(2, 1, 4, 4)), slot_of_image=mk(_z(3, dt=i32)), lambdas=mk(_z(2, 3)), sky=img(3, 4, 4),
                                                 img=mk(_z(1, dt=i64)), coords=mk(_z(5, 2, dt=i64))), set(), ("sky", _z(3, 4, 5, dt=u8)), None),
        "reproj_conf": ("ops", "reproj_conf", dict(images=img(2, 8, 8, 3), depths=mk(_z(2, 8, 8)), poses=mk(_z(2, 3, 4)), intrinsics=mk(_z(2, 4)), base=0,
                                                   neighbours=[1], modes=["rgb"], tau=.1, out=mk(_z(1, 8, 8)), ws=img(QUERY)),
                        set(), ("depths", _z(2, 8, 7)), "ws"),
        "frame_metrics": ("ops", "frame_metrics", dict(pred=mk(_z(8, 8, 3)), gt=img(8, 8, 3), out=mk(_z(1, 5, dt=f64)), ws=img(QUERY)),
                          set(), ("out", _z(2, 5, dt=f64)), "ws"),
        "mesh_prepare": ("ops", "mesh_prepare", dict(vertices=mk(_z(4, 3)), faces=mk(_z(2, 3, dt=i32)), face_ids=mk(_z(2, dt=i32)), transform=mk(_z(3, 4)),
                                                     ws=img(QUERY)), set(), ("faces", _z(2, 4, dt=i32)), "ws"),
        "mesh_trace_pinhole": ("ops", "mesh_trace_pinhole", dict(ws=img(QUERY), F=2, fx=4., fy=4., cx=2., cy=2., pixel_center=True, H=4, W=4,
                                                                 mask=img(4, 4, 3)), set(), ("mask", _z(4, 5, 3, dt=u8)), "ws"),
        "shadow_fuse": ("ops", "shadow_fuse", dict(im=img(4, 4, 3), total_mask=img(4, 4, 3), shadow_mask=img(4, 4, 3), H=4, W=4, light_scale=.5,
                                                   check=False, ws=img(QUERY)), set(), ("im", _z(4, 5, 3, dt=u8)), None),
        "handle_occlusion_paste": ("foreground", "handle_occlusion_paste", dict(bg_im=img(4, 4, 3), vehicle_im=img(4, 4, 3), mask_im=img(4, 4, 3),
                                                                                depth_mat=mk(_z(4, 4)), semantic_mat=img(4, 4), fg_depth=mk(_z(4, 4))),
                                   set(), ("semantic_mat", _z(4, 5, dt=u8)), None),
        "handle_lighting": ("foreground", "handle_lighting", dict(im=img(4, 4, 3), mask=img(4, 4, 3), stats=mk(_z(9, dt=i64))),
                            set(), ("stats", _z(8, dt=i64)), None),
        "overlap_stats": ("foreground", "overlap_stats", dict(masks=[img(4, 4, 3), img(4, 4, 3), img(4, 4, 3)]), set(), (("masks", 1), _z(4, 5, 3, dt=u8)),
                          None),
    }


CASE_IDS = sorted(_cases(_fake))


# ---- point 4 of the issue: every tensor whose hand-written chain forgot is_cuda or is_contiguous(), wrapper by wrapper, with a minimal valid
# call -> (module, function, kwargs, [tightened arguments]).  The fused-MLP lists go through the three array builders every fused entry
# shares.  (" cpu" behind a name: the argument stays a strided view or has one element, only the device check can be shown.)
def _tightened(mk):
    import numpy as np
    i32t = lambda *sh: mk(_z(*sh, dt=i32))
    rays7 = lambda: dict(tdist=mk(_z(2, 4)), origins=mk(_z(2, 3)), directions=mk(_z(2, 3)), radii=mk(_z(2, 1)), base_x=mk(_z(2, 3)), base_y=mk(_z(2, 3)),
                         deg_jitter=mk(_z(2, 3)))
    grid = dict(L=2, C=4, n=2, m=1, Sl=1., H=4, std_scale=.5)
    mip_out = lambda: dict(origins=mk(_z(4, 3)), directions=mk(_z(4, 3)), viewdirs=mk(_z(4, 3)), radii=mk(_z(4, 1)), lossmult=mk(_z(4, 1)), near=mk(_z(4, 1)),
                           far=mk(_z(4, 1)), app=mk(_z(4, 1)), rgb=mk(_z(4, 3)), sel_coords=mk(_z(4, 2, dt=i64)), img=mk(_z(1, dt=i64)))
    mip_in = lambda: dict(images=mk(_z(2, 4, 4, 3, dt=u8)), depths=mk(_z(2, 4, 4)), poses=mk(_z(2, 3, 4)), intrinsics=mk(_z(2, 4)), near=mk(_z(2)), far=mk(_z(2)),
                          app=mk(_z(2)), extras=None, i_train=i32t(2), seed=1, counter=mk(_z(2, dt=i64)), n=4, i0=0, i1=4)
    zip_out = lambda: dict({k: mk(_z(4, 3)) for k in ("origins", "directions", "viewdirs", "base_x", "base_y", "rgb")},
                           **{k: mk(_z(4, 1)) for k in ("radii", "lossmult", "near", "far", "cam_idx")}, pix_x_int=i32t(4), pix_y_int=i32t(4))
    zip_in = lambda: dict(images=mk(_z(2, 4, 4, 3, dt=u8)), depths=mk(_z(2, 4, 4)), semantics=i32t(2, 4, 4), masks=mk(_z(2, 4, 4)), pixtocams=mk(_z(2, 3, 3)),
                          camtoworlds=mk(_z(2, 3, 4)), local2global=i32t(2), near=.1, far=10., border=0, patch_size=1, single_image=False, seed=1,
                          counter=mk(_z(2, dt=i64)), n=4)
    coords = i32t(4, 2)
    t = {
        "classic_embed": ("ops", "classic_embed", dict(pts=mk(_z(4, 3)), viewdirs=mk(_z(2, 3)), S=2, L=10, Lv=4, dst1=mk(_z(4, 64)), dst2=None, w_pts=64,
                                                       dstv=mk(_z(4, 32)), w_views=32, dt=ops.F32), ["viewdirs"]),
        "fmlp_classic_pts_fwd": ("ops", "fmlp_classic_pts_fwd", dict(pts=mk(_z(4, 3)), viewdirs=mk(_z(2, 3)), S=2, stream=mk(_z(64, dt=bf16)), bias=mk(_z(32)),
                                                                     raw=mk(_z(4, 4))), ["viewdirs", "stream", "bias"]),
        "fmlp_zip_fwd": ("ops", "fmlp_zip_fwd", dict(Fb=mk(_z(2, 64, dt=bf16)), D=mk(_z(2, 16, dt=bf16)), stream=mk(_z(64, dt=bf16)), bias=mk(_z(32)),
                                                     raw_rgb=mk(_z(2, 3)), raw_d=mk(_z(2, 1))), ["stream", "bias"]),
        "_mat_arrays": ("ops", "_mat_arrays", dict(mats=[mk(_z(2, 4, dt=bf16))], M=2, widths=[4], tdt=bf16), [("mats", 0)]),
        "_mask_array": ("ops", "_mask_array", dict(bits=[i32t(4)], M=2, widths=[0]), [("bits", 0)]),
        "_bias_array": ("ops", "_bias_array", dict(g_bias=[mk(_z(4))], widths=[4]), [("g_bias", 0)]),
        "stratified": ("ops", "stratified", dict(base=mk(_z(5)), rnd=None, near=mk(_z(4)), far=mk(_z(4)), n=4, mode=0), ["near cpu", "far cpu"]),
        "classic_composite_fwd": ("ops", "classic_composite_fwd", dict(raw=mk(_z(12, 4)), noise=None, z_vals=mk(_z(4, 3)), rays_d=mk(_z(4, 3)), white=False),
                                  ["rays_d"]),
        "sgd_step": ("ops", "sgd_step", dict(p=mk(_z(8)), g=mk(_z(8)), lr=.1, clip_coef=mk(_z(2)), dropped=mk(_z(1, dt=i64))), ["clip_coef", "dropped cpu"]),
        "nonfinite_flag": ("ops", "nonfinite_flag", dict(g=mk(_z(8)), flag=i32t(2)), ["flag"]),
        "gather_pack_pair": ("ops", "gather_pack_pair", dict(flat=mk(_z(16)), idx=i32t(8), dst=mk(_z(8, dt=bf16)), tiles=i32t(2, 4), idx32=i32t(4),
                                                             dst32=mk(_z(4))), ["flat", "idx", "dst", "tiles", "idx32", "dst32"]),
        "grid_encode_bwd": ("ops", "grid_encode_bwd", dict(grad=mk(_z(4, 4)), inputs=mk(_z(4, 3)), embeddings=mk(_z(16, 2)), offsets=i32t(3), L=2, S=1., H=4,
                                                           gridtype=0, align_corners=False, interp=0), ["grad"]),
        "grid_encode_bwd_binned": ("ops", "grid_encode_bwd_binned", dict(grad=mk(_z(4, 4)), inputs=mk(_z(4, 3)), offsets=i32t(3), C=2, L=2, S=1., H=4,
                                                                         offsets_host=np.array([0, 8, 16], dtype=np.int32)), ["grad"]),
        "grid_tv_grad": ("ops", "grid_tv_grad", dict(inputs=mk(_z(4, 3)), embeddings=mk(_z(16, 2)), grad=mk(_z(16, 2)), offsets=i32t(3), weight=.1, L=2, S=1.,
                                                     H=4, gridtype=0, align_corners=False), ["grad", "embeddings"]),
        "hash_decay": ("ops", "hash_decay", dict(table=mk(_z(16, 4)), grad=mk(_z(16, 4)), offsets=i32t(3), L=2, C=4, mult=.1), ["offsets"]),
        "zip_encode_fwd": ("ops", "zip_encode_fwd", dict(rays7(), table=mk(_z(16, 4)), offsets=i32t(3), grid_sizes=i32t(2), feat=mk(_z(6, 8)), **grid),
                           ["table", "offsets", "grid_sizes"]),
        "zip_encode_fwd_count": ("ops", "zip_encode_fwd_count", dict(rays7(), table=mk(_z(16, 4)), offsets=i32t(3), grid_sizes=i32t(2), feat=mk(_z(6, 8)),
                                                                     ksplit=[1, 1], level_rows=[8, 8], **grid), ["table", "offsets", "grid_sizes"]),
        "zip_encode_prop_fwd": ("ops", "zip_encode_prop_fwd", dict(rays7(), table=mk(_z(16, 1)), offsets=i32t(3), grid_sizes=i32t(2), L=2, n=2, m=1, Sl=1., H=4,
                                                                   std_scale=.5, w1=mk(_z(8)), b1=mk(_z(4)), w2=mk(_z(4)), b2=mk(_z(1)), round_bf16=False),
                                ["table"]),
        "zip_encode_ray_bwd": ("ops", "zip_encode_ray_bwd", dict(rays7(), table=mk(_z(16, 4)), offsets=i32t(3), grid_sizes=i32t(2), grad_feat=mk(_z(6, 8)),
                                                                 g_o=mk(_z(2, 3)), g_d=mk(_z(2, 3)), g_bx=mk(_z(2, 3)), g_by=mk(_z(2, 3)), **grid),
                               ["table", "grad_feat"]),
        "zip_encode_bwd_binned": ("ops", "zip_encode_bwd_binned", dict(rays7(), offsets=i32t(3), grid_sizes=i32t(2), grad_feat=mk(_z(6, 8)),
                                                                       grad_table=mk(_z(16, 4)), ksplit=[1, 1], g64_rows=0, level_rows=[8, 8], **grid),
                                  ["grad_table"]),
        "zip_prop_mlp_bwd": ("ops", "zip_prop_mlp_bwd", dict(F=mk(_z(6, 2)), d_raw=mk(_z(6)), L=2, w1=mk(_z(8)), b1=mk(_z(4)), w2=mk(_z(4)), b2=mk(_z(1)),
                                                             round_bf16=False, g_w1=mk(_z(8)), g_b1=mk(_z(4)), g_w2=mk(_z(4)), g_b2=mk(_z(1))), ["d_raw"]),
        "colsum_wide_f32": ("ops", "colsum_wide_f32", dict(x=mk(_z(4, 8)), C=8, out=mk(_z(8))), ["out"]),
        "pinhole_rays": ("ops", "pinhole_rays", dict(coords=coords, first_pixel=0, n=4, W=4, H=4, pose=np.eye(4)[:3], cx=2., cy=2., fx=4., fy=4., training=True,
                                                     near=.1, far=10., device=coords.device), ["coords"]),
        "classic_ert_step": ("ops", "classic_ert_step", dict(raw_g=mk(_z(4, 2, 4)), alive=None, z_all=mk(_z(4, 3)), rays=mk(_z(4, 8)), g0=0, G=2, eps_t=1e-4,
                                                             T=mk(_z(4)), raw_full=mk(_z(4, 3, 4)), scratch=(i32t(4), i32t(4), i32t(4), mk(_z(1, dt=i64)))),
                             ["raw_g", "raw_full"]),
        "zip_pixels_to_rays": ("ops", "zip_pixels_to_rays", dict(pix_x=i32t(4), pix_y=i32t(4), cam_idx=i32t(4), pixtocams=mk(_z(2, 3, 3)),
                                                                 camtoworlds=mk(_z(2, 3, 4))), ["pix_x", "pix_y", "cam_idx"]),
        "mip_image_batch": ("ops", "mip_image_batch", dict(mip_in(), out=mip_out()), ["i_train", "counter"]),
        "mip_image_patch_batch": ("ops", "mip_image_patch_batch", dict(mip_in(), n_patch=0, patch_sz=2, k0=0, k1=0, out=mip_out()), ["i_train", "counter"]),
        "zip_ray_batch": ("ops", "zip_ray_batch", dict(zip_in(), i0=0, i1=4, out=zip_out()), ["semantics", "local2global", "counter"]),
        "zip_ray_patch_batch": ("ops", "zip_ray_patch_batch", dict(zip_in(), k0=0, k1=0, i0=0, i1=4, out=zip_out()), ["semantics", "local2global", "counter"]),
        "zip_loss_tail": ("ops", "zip_loss_tail", dict(rgb=mk(_z(4, 3)), tgt=mk(_z(4, 3)), sem=mk(_z(4, 2)), labels=i32t(4)), ["labels"]),
        "semantic_composite_fwd": ("ops", "semantic_composite_fwd", dict(weights=mk(_z(4, 3)), logits=mk(_z(12, 2)), C=2, softmax=True, row_index=i32t(4, 3)),
                                   ["row_index"]),
    }
    for cid, args in (("linear_fwd_bits", ["aux"]), ("fmlp_proposal_fwd", ["stream", "bias", "raw_density"]), ("adam_step", ["clip_coef"]),
                      ("gather_pack", ["flat", "idx", "dst", "tiles"]), ("grid_encode_fwd", ["offsets"]),
                      ("zip_encode_bwd", ["grad_table", "grad_table_bf16"]), ("handle_occlusion_paste", ["fg_depth"])):
        t[cid] = _cases(mk)[cid][:3] + (args,)
    return t


TIGHTENED_IDS = sorted(_tightened(_fake))


def _positions(kw):
    """the tensor arguments of a call: names, or (name, index) for a list of tensors"""
    out = []
    for k, v in kw.items():
        if torch.is_tensor(v):
            out.append(k)
        elif isinstance(v, list) and v and torch.is_tensor(v[0]):
            out += [(k, i) for i in range(len(v))]
    return out


def _get(kw, pos):
    return kw[pos] if isinstance(pos, str) else kw[pos[0]][pos[1]]


def _with(kw, pos, value):
    kw = dict(kw)
    if isinstance(pos, str):
        kw[pos] = value
    else:
        kw[pos[0]] = list(kw[pos[0]])
        kw[pos[0]][pos[1]] = value
    return kw


def _name(pos):
    return pos if isinstance(pos, str) else pos[0]


class _Stub:
    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))

    def query(self, name, *args):
        return QUERY


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(_lib, "call", s.call)
    monkeypatch.setattr(_lib, "query", s.query)
    for mod in (ops, foreground):
        monkeypatch.setattr(mod, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_zeros_cache", {})
    monkeypatch.setattr(ops, "_zb_ws", {})
    return s


class _OptimizedLoader(importlib.machinery.SourceFileLoader):
    """compiles a module as `python -OO` would (asserts and docstrings gone), past the bytecode cache in both directions"""

    def get_code(self, fullname):
        path = self.get_filename(fullname)
        return compile(self.get_data(path), path, "exec", dont_inherit=True, optimize=2)


def _load_optimized(name):
    full = f"snerf_amd._{name}_optimized"
    spec = importlib.util.spec_from_loader(full, _OptimizedLoader(full, os.path.join(os.path.dirname(snerf_amd.__file__), name + ".py")))
    mod = importlib.util.module_from_spec(spec)                 # (__package__ = snerf_amd: `from . import _lib` is the stubbed module)
    spec.loader.exec_module(mod)
    assert mod.__doc__ is None and mod.__name__ == full          # optimize=2 took the docstring: the compile above is the one that ran
    return mod


def _refusals(mods, mk, stub, mutate):
    """every tensor argument of every case replaced by mutate(case's valid tensor) -> [(case, argument, exception type, message)]"""
    out = []
    for cid, (mod, fn, kw, loose, _, _) in sorted(_cases(mk).items()):
        for pos in _positions(kw):
            bad = mutate(_get(kw, pos), _name(pos) in loose)
            if bad is None:
                continue
            with pytest.raises(_lib.SnerfArgumentError) as e:
                getattr(mods[mod], fn)(**_with(kw, pos, bad))
            assert re.search(rf"\b{_name(pos)}\b", str(e.value)), (cid, pos, str(e.value))
            assert isinstance(e.value, ValueError) and isinstance(e.value, AssertionError)
            assert stub.calls == [], (cid, pos, stub.calls)
            out.append((cid, pos, type(e.value).__name__, str(e.value)))
    return out


def _on_cpu(t, loose):
    return t.as_subclass(torch.Tensor).cpu()


# ------------------------------------------------------------------------------------------------------- no GPU, no library ----------
def test_no_assert_statement_is_left_in_the_binding_layer():
    for name in MODULES:
        path = os.path.join(os.path.dirname(snerf_amd.__file__), name + ".py")
        found = [n.lineno for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Assert)]
        assert found == [], (name, found)


def test_the_error_type_is_a_value_error_and_an_assertion_error():
    assert issubclass(_lib.SnerfArgumentError, ValueError) and issubclass(_lib.SnerfArgumentError, AssertionError)
    assert not issubclass(_lib.SnerfArgumentError, _lib.SnerfHipError) and not issubclass(_lib.SnerfHipError, ValueError)


def test_a_cpu_tensor_is_refused_in_every_tensor_position(stub):
    got = _refusals(dict(ops=ops, foreground=foreground), _fake, stub, _on_cpu)
    assert {c for c, *_ in got} == set(CASE_IDS) and len(got) >= 100


def test_the_refusals_are_the_same_when_compiled_as_python_O_would(stub, monkeypatch):
    plain = _refusals(dict(ops=ops, foreground=foreground), _fake, stub, _on_cpu)
    ops_o, fg_o = _load_optimized("ops"), _load_optimized("foreground")
    for name in ("_dev", "_require", "_p"):                      # the optimized foreground runs on the optimized checkers
        setattr(fg_o, name, getattr(ops_o, name))
    for mod in (ops_o, fg_o):
        monkeypatch.setattr(mod, "_stream", lambda: 0)
    assert _refusals(dict(ops=ops_o, foreground=fg_o), _fake, stub, _on_cpu) == plain


def test_a_valid_call_passes_the_checks_without_a_gpu(stub):
    """the table's valid calls are valid: each reaches the stub once (guards the refusal tests against a table that is refused anyway)"""
    for cid, (mod, fn, kw, _, _, _) in sorted(_cases(_fake).items()):
        del stub.calls[:]
        getattr(dict(ops=ops, foreground=foreground)[mod], fn)(**kw)
        assert len(stub.calls) == 1, (cid, stub.calls)


def _check_tightened(mk, stub, cid, to_cpu):
    """the valid call of the case passes; each tightened argument on the CPU or as a non-contiguous view is refused, by its name"""
    mod, fn, kw, args = _tightened(mk)[cid]
    f = getattr(dict(ops=ops, foreground=foreground)[mod], fn)
    f(**kw)
    del stub.calls[:]
    for arg in args:
        pos, cpu_only = (arg[:-4], True) if isinstance(arg, str) and arg.endswith(" cpu") else (arg, False)
        t = _get(kw, pos)
        assert cpu_only or t.numel() > 1, (cid, arg)
        for bad in (to_cpu(t), None if cpu_only else _non_contiguous(t, False)):
            if bad is not None:
                with pytest.raises(_lib.SnerfArgumentError, match=rf"\b{_name(pos)}\b"):
                    f(**_with(kw, pos, bad))
    assert stub.calls == [], (cid, stub.calls)


@pytest.mark.parametrize("cid", TIGHTENED_IDS)
def test_the_tightened_tensors_are_refused_without_a_gpu(stub, cid):
    _check_tightened(_fake, stub, cid, lambda t: _on_cpu(t, False))


# ------------------------------------------------------------------------------------- device tensors, the stubs still in place ----------
def _wrong_dtype(t, loose):
    return None if loose else t.to(torch.int16)


def _non_contiguous(t, loose):
    if loose or t.numel() < 2:                                    # (a one-element tensor is contiguous whatever its strides say)
        return None
    v = torch.stack([t, t], dim=-1)[..., 0]
    assert v.shape == t.shape and not v.is_contiguous()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("mutate", [_on_cpu, _wrong_dtype, _non_contiguous], ids=["cpu", "dtype", "non_contiguous"])
def test_device_tensors_of_the_wrong_kind_are_refused(stub, mutate):
    got = _refusals(dict(ops=ops, foreground=foreground), _real, stub, mutate)
    assert {c for c, *_ in got} == set(CASE_IDS)


@pytest.mark.gpu
def test_wrong_shapes_and_short_workspaces_are_refused(stub):
    mods = dict(ops=ops, foreground=foreground)
    shapes = sizes = 0
    for cid, (mod, fn, kw, _, wrong_shape, short_ws) in sorted(_cases(_real).items()):
        if wrong_shape is not None:
            pos, bad = wrong_shape
            with pytest.raises(_lib.SnerfArgumentError):
                getattr(mods[mod], fn)(**_with(kw, pos, bad.cuda()))
            shapes += 1
        if short_ws is not None:
            with pytest.raises(_lib.SnerfArgumentError, match=r"\bws\b"):
                getattr(mods[mod], fn)(**_with(kw, short_ws, kw[short_ws][:QUERY - 1]))
            sizes += 1
        assert stub.calls == [], (cid, stub.calls)
    assert shapes == len(CASE_IDS) - 2 and sizes == 4


def _flat(args):
    for a in args:
        if isinstance(a, ctypes.Array):
            yield from list(a)
        else:
            yield a


@pytest.mark.gpu
def test_a_valid_call_reaches_the_library_once_with_the_tensors_pointers(stub):
    mods = dict(ops=ops, foreground=foreground)
    for cid, (mod, fn, kw, _, _, _) in sorted(_cases(_real).items()):
        del stub.calls[:]
        getattr(mods[mod], fn)(**kw)
        assert len(stub.calls) == 1, (cid, stub.calls)
        args = list(_flat(stub.calls[0][1]))
        for pos in _positions(kw):
            assert _get(kw, pos).data_ptr() in args, (cid, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", TIGHTENED_IDS)
def test_the_tensors_whose_checks_were_tightened_are_refused(stub, cid):
    _check_tightened(_real, stub, cid, lambda t: t.cpu())
