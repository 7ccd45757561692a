"""The C-ABI shared library loads without a GPU and exports every symbol include/snerf_hip.h declares."""
import ctypes
import os
import re

import pytest

from snerf_amd import _lib


def test_header_parses_and_lists_entry_points():
    protos = _lib.parse_header()
    src = open(_lib.HEADER_PATH).read()
    declared = set(re.findall(r"\b(?:int|long)\s+(snerf_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", src, flags=re.S)))
    assert declared == set(protos) and len(protos) >= 18
    for name in ("snerf_linear_fwd", "snerf_linear_wgrad", "snerf_mip_encode", "snerf_mip_resample", "snerf_classic_sample_pdf",
                 "snerf_mip_composite_fwd", "snerf_mip_composite_bwd", "snerf_classic_composite_fwd", "snerf_adam_step"):
        assert name in protos
    # no torch / C++ types in the signatures: only pointers and plain scalars
    for sig in protos.values():
        for ty, _ in sig:
            assert ty in (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnerf_hip.so not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    for name in _lib.parse_header():
        assert getattr(lib, name) is not None
    assert lib.snerf_version() >= 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        _lib.load()


def test_bad_arguments_are_rejected_without_a_gpu():
    """argument validation happens before any launch, so it can be exercised on a CPU-only box"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        _lib.call("snerf_linear_fwd", None, 0, None, 0, None, None, 0, None, 0, None, None, 16, 100, 64, 1, 0, 1, 0, 0, None)  # N % 128 != 0
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        _lib.call("snerf_mip_resample", None, None, None, 0, 4, 1, 8, 0.01, None, None, None)  # S < 2
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        _lib.call("snerf_jitter_u", None, 4, 8, 0.125, None)                                   # no buffer
    with pytest.raises(_lib.SnerfHipError, match="bad argument"):
        _lib.call("snerf_gather_pack_tiles", None, None, 16, None, 1, None, 1, None)           # no arena / map / destination
    assert _lib.call("snerf_jitter_u", None, 0, 8, 0.125, None) is None                        # an empty batch is not an error


def test_no_vector_alu_instruction_hides_in_inline_asm():
    """A VALU result needs wait states before an MFMA reads it; hipcc counts them for the instructions it emits itself but not for the
    text of an inline asm (round 2: an inline `v_pk_max_i16` in front of an MFMA gave rare, timing-dependent wrong results in one
    instantiation of the fused MLP kernel; tools/probes/mfma_war_probe.hip shows the hazard in isolation).  Inline asm in the kernels is
    therefore limited to waits, barriers, scalar / debug register reads, the transposing LDS read and (round 3) the input-row loads of
    the fused colour head (memory instructions, both waited for by hand with the destination registers as operands of the wait), the LDS
    atomic add of the fused gradient chains' bias-gradient table and empty optimisation fences."""
    import glob
    import re
    allowed = ("s_waitcnt", "s_barrier", "s_lshr_b32", "s_getreg_b32", "ds_read_b64_tr_b16", "ds_read_b32", "ds_read_b128", "ds_add_f32", "ds_add_u32", "global_load_dwordx4", "s_nop", "s_sleep", ";")
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "snerf_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h"))):
        src = open(path).read()
        for m in re.finditer(r'\basm\s*(?:volatile)?\s*\(\s*((?:"[^"]*"\s*)+)', src):
            text = "".join(re.findall(r'"([^"]*)"', m.group(1)))
            for ins in re.split(r"\\n\\t|\\n|\\t", text):
                ins = ins.strip()
                if ins:
                    assert ins.startswith(allowed), f"{os.path.basename(path)}: inline asm instruction {ins!r}"


def test_grid_binned_backward_workspace_query_and_its_limits():
    """snerf_grid_encode_bwd_binned_ws_bytes / _plan are host-only: the recommended workspace is BOUNDED (at most 1 GiB at the bench's 14.7 M
    points, where the round-5 form needed 11-30 GB: at most 1 GB), smaller workspaces plan more chunks, -1 for what the binned kernels do not cover
    (C not in {1, 2, 4, 8}, a level with more than 1024 row ranges) -- GridEncoder.backward then falls back to the atomic scatter."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    import numpy as np
    import torch
    from snerf_amd import ops
    q = lambda B, C, off, half: _lib.query("snerf_grid_encode_bwd_binned_ws_bytes", B, C, len(off) - 1, np.ascontiguousarray(np.asarray(off, dtype=np.int32)).ctypes.data, half)
    off, _ = ops.grid_level_layout(3, 10, ops.grid_per_level_scale(16, 8192, 10), 16, 21)
    B = 65536 * 32 * 7
    full = q(B, 4, off, 1)
    assert 0.5e9 < full <= 1e9 and q(B, 4, off, 0) <= 1e9
    plan = ops.grid_encode_bwd_binned_plan(B, 4, 10, off, True, torch.float16)
    assert plan["bytes_used"] <= full and plan["chunks"] >= 2 and 1 <= plan["levels_per_transposed_group"] <= 10 and plan["launches"] < 400
    assert plan["chunk_record_capacity"] >= 8 * plan["chunk_points"]
    lm = ops.grid_encode_bwd_binned_plan(B, 4, 10, off, True, torch.float16, level_major=True)
    assert lm["levels_per_transposed_group"] == 0 and lm["chunks"] <= plan["chunks"]          # the reference's layout needs no transposed copy
    small = ops.grid_encode_bwd_binned_plan(B, 4, 10, off, True, torch.float16, ws_bytes=300 << 20)
    assert small["bytes_used"] <= (300 << 20) and small["chunks"] > plan["chunks"]
    few = ops.grid_encode_bwd_binned_plan(20000, 4, 10, off, True, torch.float16)
    assert few["chunks"] == 1 and few["levels_per_transposed_group"] == 10 and few["bytes_used"] < (64 << 20)
    assert q(1000, 1, off, 1) > 0 and q(0, 4, off, 1) == 0
    assert q(1000, 2, off, 0) > 0 and q(1000, 8, off, 1) > 0 and q(1000, 3, off, 0) == -1
    big = [0, 8, 8 + (1 << 23)]                                                   # 2^23 rows at C = 4: 2048 row ranges of 4096
    assert q(1000, 4, big, 1) == -1 and q(1000, 8, big, 0) == -1 and q(1000, 1, big, 1) > 0    # (C = 1: 512 ranges of 16384)


# ---- the host statuses of the fused entries (csrc/fmlp.hip), one case list per entry ---------------------------------------------------------
# Every case below is one that validation refuses or that has M <= 0: nothing reaches a launch, so the list runs on a box without a GPU.
_F32, _BF16, _F16 = 0, 1, 2
_HOST = (ctypes.c_char * 64)()
_A = (ctypes.addressof(_HOST) + 15) & ~15           # a 16-byte aligned host address: the checks never dereference it
_BIG = 1 << 31


def _mats(ptr, ld, widths, min_width=True):
    """refusals of an array of stored 16-bit matrices: null / misaligned pointer, stride % 8, stride below the width the entry asks for"""
    out = []
    for i, w in enumerate(widths):
        out += [{f"{ptr}[{i}]": None}, {f"{ptr}[{i}]": _A + 8}, {f"{ld}[{i}]": w + 4}]
        if min_width:
            out.append({f"{ld}[{i}]": w - 8})
    return out + [{ptr: None}, {ld: None}]


def _ptrs(name, n, aligned):
    """refusals of an array of bit-mask (aligned) or bias-gradient pointers"""
    return [{f"{name}[{i}]": None} for i in range(n)] + ([{f"{name}[{i}]": _A + 4} for i in range(n)] if aligned else []) + [{name: None}]


def _nulls(*names):
    return [{n: None} for n in names]


_W10 = [256] * 9 + [128]
_CLASSIC = dict(wstream=_A, n_frags=1184, bias=_A, n_blocks=78, raw=_A, M=256)
_STREAM_256 = _nulls("wstream", "bias", "raw") + [{"wstream": _A + 8}, {"n_frags": 1168}, {"n_frags": 1200}, {"n_blocks": 77}]
_ROWS = dict(_CLASSIC, E=_A, ldE=64, VE=_A, ldVE=32)
_ROWS_BAD = _STREAM_256 + _nulls("E", "VE") + [{"E": _A + 8}, {"VE": _A + 8}, {"ldE": 68}, {"ldVE": 36}, {"raw": _A + 4}]
_TRAIN = dict(acts=[_A] * 10, act_ld=_W10, bits=[_A] * 9)
_TRAIN_BAD = _mats("acts", "act_ld", _W10, min_width=False) + _ptrs("bits", 9, True)
_X = dict(_CLASSIC, x=_A, ldx=90)
_X_BAD = _STREAM_256 + [{"x": None}, {"x": _A + 2}, {"ldx": 89}, {"raw": _A + 4}, {"M": _BIG}]
_PROP = dict(E=_A, ldE=96, wstream=_A, n_frags=448, bias=_A, n_blocks=33, raw_density=_A, M=256)
_PROP_BAD = _nulls("E", "wstream", "bias", "raw_density") + [{"E": _A + 8}, {"ldE": 100}, {"wstream": _A + 8}, {"n_frags": 432}, {"n_blocks": 32}]
_ZIP = dict(F=_A, ldF=64, D=_A, ldD=16, wstream=_A, n_frags=464, bias=_A, n_blocks=35, raw_rgb=_A, ld_rgb=3, raw_d=_A, ld_d=1, M=256)
_ZIP_BAD = _nulls("F", "D", "wstream", "bias", "raw_rgb", "raw_d") + [
    {"ldF": 56}, {"ldD": 8}, {"ldF": 68}, {"ldD": 20}, {"F": _A + 8}, {"D": _A + 8}, {"ld_rgb": 2}, {"ld_d": 0}, {"M": _BIG}, {"n_blocks": 34},
    {"n_frags": 460}, {"n_frags": 448}]
_COLOUR_BWD = dict(d_raw_rgb=_A, wstream=_A, n_frags=336, bits=[_A] * 4, dC=[_A] * 3, dC_ld=[128] * 3, dB=_A, dB_ld=1024, g_bias=[_A] * 4, ws=_A,
                   ws_floats=1 << 40, M=256)
_CHAIN = dict(d_raw=_A, wstream=_A, ws=_A, ws_floats=1 << 40, M=256)
_CHAIN_BAD = _nulls("d_raw", "wstream", "ws") + [{"wstream": _A + 8}, {"d_raw": _A + 8}, {"ws_floats": "short"}, {"n_frags": 416}]

# entry (the `_dt` name where there is a bf16 twin) -> (arguments that would reach the launch, refusals: each changes the arguments named)
_FUSED = {
    "snerf_fmlp_classic_fwd_dt": (_ROWS, _ROWS_BAD),
    "snerf_fmlp_classic_train_fwd_dt": (dict(_ROWS, **_TRAIN), _ROWS_BAD + _TRAIN_BAD),
    "snerf_fmlp_classic_pts_fwd_dt": (dict(_CLASSIC, pts=_A, viewdirs=_A, ldvd=3, S=8),
                                      _STREAM_256 + _nulls("pts", "viewdirs") + [{"S": 0}, {"ldvd": 2}, {"raw": _A + 4}, {"M": _BIG}]),
    "snerf_fmlp_classic_x_fwd_dt": (_X, _X_BAD),
    "snerf_fmlp_classic_x_train_fwd_dt": (dict(_X, xin=[_A] * 3, xin_ld=[64, 64, 32], **_TRAIN),
                                          _X_BAD + _mats("xin", "xin_ld", [64, 64, 32]) + _TRAIN_BAD),
    "snerf_fmlp_proposal_fwd_dt": (_PROP, _PROP_BAD),
    "snerf_fmlp_proposal_train_fwd_dt": (dict(_PROP, acts=[_A] * 4, act_ld=[256] * 4, bits=[_A] * 4),
                                         _PROP_BAD + _mats("acts", "act_ld", [256] * 4, min_width=False) + _ptrs("bits", 4, False)),
    "snerf_fmlp_zip_fwd": (dict(_ZIP, x32=None, ld_x=0),
                           _ZIP_BAD + [{"x32": _A, "ld_x": 28}, {"x32": _A, "ld_x": 34}, {"x32": _A + 4, "ld_x": 32}]),
    "snerf_fmlp_zip_train_fwd": (dict(_ZIP, acts=[_A] * 4, act_ld=[64, 256, 256, 256], bits=[_A] * 3),
                                 _ZIP_BAD + _mats("acts", "act_ld", [64, 256, 256, 256]) + _ptrs("bits", 3, True)),
    "snerf_fcolour_fwd_dt": (dict(CB=_A, ldCB=1056, wstream=_A, n_frags=336, bias=_A, n_blocks=13, raw_rgb=_A, acts=[_A] * 3, act_ld=[128] * 3,
                                  bits=[_A] * 3, M=256, variant=0),
                             _nulls("CB", "wstream", "bias", "raw_rgb") + [{"CB": _A + 8}, {"wstream": _A + 8}, {"ldCB": 1060}, {"ldCB": 1048},
                                                                            {"n_frags": 320}, {"n_blocks": 12}, {"variant": 1, "n_blocks": 14}]
                             + [c for c in _mats("acts", "act_ld", [128] * 3) if c != {"acts": None}] + _ptrs("bits", 3, False)),
    "snerf_fcolour_bwd_dt": (_COLOUR_BWD,
                             _nulls("d_raw_rgb", "wstream", "dB", "ws") + [{"n_frags": 320}, {"wstream": _A + 8}, {"dB": _A + 8}, {"dB_ld": 1028},
                                                                           {"dB_ld": 1016}, {"ws_floats": "short"}, {"M": _BIG // 12 + 1},
                                                                           {"d_raw_rgb": _A + 8}]
                             + _ptrs("bits", 4, True) + _mats("dC", "dC_ld", [128] * 3) + _ptrs("g_bias", 4, False)),
    "snerf_fchain_bwd_dt": (dict(_CHAIN, net=0, n_frags=1104, bits=[_A] * 9, dz=[_A] * 10, dz_ld=[128] + [256] * 9, g_bias=[_A] * 10),
                            _CHAIN_BAD + [{"net": 2}, {"net": -1}, {"n_frags": 400}, {"M": _BIG // 16}] + _ptrs("bits", 9, True)
                            + _mats("dz", "dz_ld", [128] + [256] * 9) + _ptrs("g_bias", 10, False)),
    "snerf_fchain_bwd_dt proposal": (dict(_CHAIN, net=1, n_frags=400, bits=[_A] * 4, dz=[_A] * 4, dz_ld=[256] * 4, g_bias=[_A] * 4),
                                     _CHAIN_BAD + [{"n_frags": 1104}, {"M": _BIG // 4}] + _ptrs("bits", 4, True) + _mats("dz", "dz_ld", [256] * 4)
                                     + _ptrs("g_bias", 4, False)),
    "snerf_fmlp_zip_chain_bwd": (dict(d_rgb=_A, ld_rgb=3, d_den=_A, ld_den=1, den_cols=1, wstream=_A, n_frags=448, bits=[_A] * 3, dz=[_A] * 5,
                                      dz_ld=[256, 256, 256, 64, 64], g_bias=[_A] * 4, ws=_A, ws_floats=1 << 40, M=256),
                                 _nulls("d_rgb", "d_den", "wstream", "ws") + [{"ld_rgb": 2}, {"den_cols": 0}, {"den_cols": 33, "ld_den": 33},
                                                                              {"den_cols": 4, "ld_den": 3}, {"n_frags": 464}, {"wstream": _A + 8},
                                                                              {"ws_floats": "short"}, {"M": _BIG}]
                                 + _ptrs("bits", 3, True) + _mats("dz", "dz_ld", [256, 256, 256, 64, 64]) + _ptrs("g_bias", 4, False)),
}
_WS_QUERY = {"snerf_fcolour_bwd_dt": lambda a: ("snerf_fcolour_bwd_ws_floats", a["M"]),
             "snerf_fchain_bwd_dt": lambda a: ("snerf_fchain_bwd_ws_floats", a["net"], a["M"]),
             "snerf_fmlp_zip_chain_bwd": lambda a: ("snerf_fmlp_zip_chain_ws_floats", a["M"])}


def _fused_status(name, values, dtype):
    """the raw status of entry `name` for the named argument values (lists become host arrays); dtype None: the twin without the argument"""
    sig, keep, args = _lib.parse_header()[name], [], []
    for _, arg in sig:
        if arg == "stream":
            args.append(None)
        elif arg == "dtype":
            args.append(dtype)
        elif isinstance(values[arg], list):
            keep.append(((ctypes.c_long if arg.endswith("_ld") else ctypes.c_void_p) * len(values[arg]))(*values[arg]))
            args.append(ctypes.addressof(keep[-1]))
        else:
            args.append(values[arg])
    return getattr(_lib.load(), name)(*args)


def _changed(name, base, change):
    values = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
    for key, v in change.items():
        if v == "short":
            v = _lib.query(*_WS_QUERY[name](values)) - 1
        if key.endswith("]"):
            arr, i = key[:-1].split("[")
            values[arr][int(i)] = v
        else:
            values[key] = v
    return values


@pytest.mark.parametrize("entry", sorted(_FUSED))
def test_fused_entries_keep_their_statuses_without_a_gpu(entry):
    """Every status-returning fused entry of csrc/fmlp.hip: each refusal it has (a dtype the kernels do not have; a null or misaligned pointer
    in each array; a stride that is no multiple of 8 or is below the width asked for; wrong n_frags / n_blocks; M >= 2^31 where checked; a
    short workspace) is "bad argument" in both 16-bit flavours and through the bf16 twin, and an empty batch is OK -- with the two precedences:
    a `_dt` entry refuses a bad dtype before it looks at M, the three zip entries return OK for M <= 0 before they look at anything."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    name = entry.split()[0]
    base, refusals = _FUSED[entry]
    twin = name[:-3] if name.endswith("_dt") else None
    assert len(refusals) == len({repr(sorted(c.items())) for c in refusals})
    for change in refusals:
        values = _changed(name, base, change)
        for dt in (_BF16, _F16):
            assert _fused_status(name, values, dt) == 1, (name, dt, change)
        if twin:
            assert _fused_status(twin, values, None) == 1, (twin, change)
    nothing = {k: (None if isinstance(v, list) or v == _A else v) for k, v in base.items()}     # no pointer at all ...
    for M in (0, -1):
        for values in (dict(base, M=M), dict(nothing, M=M), dict(nothing, M=M, n_frags=0, n_blocks=0)):    # ... is fine for an empty batch
            for dt in (_BF16, _F16):
                assert _fused_status(name, values, dt) == 0, (name, dt, M)
            if twin:
                assert _fused_status(twin, values, None) == 0, (twin, M)
    for dt in (_F32, 3, 4, 5, -1):
        assert _fused_status(name, base, dt) == 1, (name, dt)
        assert _fused_status(name, dict(base, M=0), dt) == (1 if twin else 0), (name, dt)       # the precedence of dtype and M
        assert _fused_status(name, dict(nothing, M=-1), dt) == (1 if twin else 0), (name, dt)


def test_fused_workspace_queries_without_a_gpu():
    """the three workspace queries: 0 for an empty batch (and an unknown net); one / two tiles of 256 rows below any CU count"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    q = _lib.query
    assert [q("snerf_fcolour_bwd_ws_floats", M) for M in (-1, 0, 1, 256, 257, 512)] == [0, 0, 1408, 1408, 2816, 2816]
    assert [q("snerf_fmlp_zip_chain_ws_floats", M) for M in (-1, 0, 1, 256, 257)] == [0, 0, 960, 960, 1856]
    assert [q("snerf_fchain_bwd_ws_floats", 0, M) for M in (0, 256, 257)] == [0, 2432 + 64, 2 * 2432 + 64]
    assert [q("snerf_fchain_bwd_ws_floats", 1, M) for M in (0, 256, 257)] == [0, 1024 + 64, 2 * 1024 + 64]
    assert q("snerf_fchain_bwd_ws_floats", 2, 256) == 0 and q("snerf_fchain_bwd_ws_floats", -1, 256) == 0
    many = q("snerf_fcolour_bwd_ws_floats", 1 << 24)                  # more tiles than CUs: the grid stops at the CU count
    assert many % 1408 == 0 and many == q("snerf_fcolour_bwd_ws_floats", 1 << 25)
    assert q("snerf_fchain_bwd_ws_floats", 1, 1 << 24) == many // 1408 * 1024 + 64
    assert q("snerf_fmlp_zip_chain_ws_floats", 1 << 24) == many // 1408 * 896 + 64


# ---- the host statuses of the GEMM entries (csrc/gemm.hip) -----------------------------------------------------------------------------------
_GEMM_M, _GEMM_N = 300, 256
# snerf_linear_fwd over (dtype, variant) x (K in 128, 192, 256) x (act 0 .. 4) x (without, with column sums), M = 300, N = n_store = 256, a 16-bit
# output: `x` = refused ("bad argument"), `.` = reaches a launch.  Read off the library before its launch code was folded into one table.
_FWD_OTHER = "......xxxx" * 3          # no persistent kernel: no bit-mask activations
_FWD_P8 = ".......x.." * 3             # the persistent kernel: everything but ReLU + bit mask with column sums
_FWD_F8 = ".x.xxxxxxx" * 3             # fp16 + fp8: forward activations only, no column sums
_FWD_REFUSED = {(dt, v): (_FWD_F8 if dt == 5 else _FWD_OTHER) for dt in (0, 1, 2, 4, 5) for v in (0, 1, 4, 8)}
_FWD_REFUSED.update({(1, 8): _FWD_P8, (2, 8): _FWD_P8, (4, 8): _FWD_P8, (5, 8): ".x.xxx.xxx" * 3})


def _gemm_ptr(mib=4):
    """one buffer for EVERY operand of a case below: a zeroed device allocation of `mib` MiB where there is a GPU -- an accepted case, and a refused
    one that a regression accepts, then runs on real memory --, else the aligned host address no refusal looks behind.  All pointers of a call
    alias that one buffer on purpose: every layout in the lists fits into it, so whatever a kernel reads or writes stays inside the allocation;
    the values it computes mean nothing and are not looked at (these tests are about statuses and launchability)."""
    import torch
    if not torch.cuda.is_available():
        return _A, None
    buf = torch.zeros(mib << 18, dtype=torch.float32, device="cuda")
    return buf.data_ptr(), buf


def _linear_fwd_status(P, dt, variant, K, act, cs, **over):
    N = _GEMM_N
    a = dict(A=P, lda=2 * K if dt in (4, 5) else K, W=P, ldw=3 * K if dt == 4 else 2 * K if dt == 5 else K, bias=None if act in (2, 4) else P,
             Y=P, ldy=N if dt == 0 else 2 * N, aux=P if act >= 2 else None, ldaux=256 if act == 2 else 0, colsum=P if cs else None,
             colsum_ws=P if cs else None, M=_GEMM_M, N=N, K=K, n_store=N, act=act, dtype=dt, out_f32=0, variant=variant, stream=None)
    a.update(over)
    return _lib.load().snerf_linear_fwd(*[a[name] for _, name in _lib.parse_header()["snerf_linear_fwd"]])


def test_linear_fwd_keeps_its_refusals():
    """snerf_linear_fwd refuses exactly the recorded (dtype, variant, K, act, column sums) combinations -- 258 of 600 -- and every
    single-argument refusal it has; M <= 0 is OK before anything is looked at.  What is not refused reaches a launch ("launch failed"
    without a device), so those cases get real device buffers where there is a GPU, and there every one of them launches."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    P, keep = _gemm_ptr()
    n_refused = 0
    for (dt, v), row in sorted(_FWD_REFUSED.items()):
        cases = [(K, act, cs) for K in (128, 192, 256) for act in range(5) for cs in (False, True)]
        for (K, act, cs), mark in zip(cases, row):
            rc = _linear_fwd_status(P, dt, v, K, act, cs)
            assert rc == (1 if mark == "x" else 2 if keep is None else 0), (dt, v, K, act, cs, rc)
            n_refused += rc == 1
    assert n_refused == 258
    if keep is not None:
        import torch
        torch.cuda.synchronize()
    bf16_p8 = dict(dt=1, variant=8, K=128)
    for what, case in {
            "N % 128": dict(dt=1, variant=0, K=128, act=0, cs=False, N=192, n_store=192),
            "N <= 0": dict(dt=1, variant=0, K=128, act=0, cs=False, N=0),
            "n_store > N": dict(dt=1, variant=0, K=128, act=0, cs=False, n_store=264),
            "n_store <= 0": dict(dt=1, variant=0, K=128, act=0, cs=False, n_store=0),
            "K % 64 (16-bit)": dict(dt=1, variant=0, K=96, act=0, cs=False),
            "K % 32 (fp32)": dict(dt=0, variant=0, K=80, act=0, cs=False),
            "K % 64 (split)": dict(dt=4, variant=8, K=96, act=0, cs=False),
            "lda % 8": dict(dt=1, variant=0, K=128, act=0, cs=False, lda=132),
            "ldw % 8": dict(dt=1, variant=0, K=128, act=0, cs=False, ldw=132),
            "unknown dtype": dict(dt=3, variant=0, K=128, act=0, cs=False),
            "unknown act": dict(dt=1, variant=0, K=128, act=5, cs=False),
            "mask without aux": dict(dt=1, variant=0, K=128, act=2, cs=False, aux=None),
            "mask with a bias": dict(dt=1, variant=0, K=128, act=2, cs=False, bias=P),
            "misaligned bit mask (producer)": dict(bf16_p8, act=3, cs=False, aux=P + 2),
            "misaligned bit mask (consumer)": dict(bf16_p8, act=4, cs=False, aux=P + 2),
            "det without the 16-byte epilogue (ldy)": dict(dt=1, variant=256, K=128, act=0, cs=True, ldy=516),
            "det without the 16-byte epilogue (no workspace)": dict(dt=1, variant=256, K=128, act=0, cs=True, colsum_ws=None),
            "det without the 16-byte epilogue (ablation bit)": dict(dt=1, variant=256 | 128, K=128, act=0, cs=True),
            "bit mask: no persistent variant": dict(dt=1, variant=4, K=128, act=3, cs=False),
            "bit mask: N % 256": dict(bf16_p8, act=3, cs=False, N=384, n_store=384, ldy=768),
            "bit mask: K < 128": dict(dt=1, variant=8, K=64, act=3, cs=False),
            "bit mask: no 16-byte epilogue": dict(bf16_p8, act=4, cs=False, n_store=252),
            "bit mask: fp32": dict(dt=0, variant=8, K=128, act=3, cs=False),
            "split mask source with split operands": dict(dt=4, variant=8 | 1 << 14, K=128, act=2, cs=False),
            "split mask source without a mask": dict(dt=1, variant=1 << 14, K=128, act=0, cs=False),
            "fp16 + fp8: partial 64-column group": dict(dt=5, variant=8, K=256, act=0, cs=False, n_store=200),
    }.items():
        assert _linear_fwd_status(P, case.pop("dt"), case.pop("variant"), case.pop("K"), case.pop("act"), case.pop("cs"), **case) == 1, what
    for M in (0, -1):                                                 # an empty batch: OK whatever else is passed
        assert _linear_fwd_status(None, 1, 0, 128, 0, False, M=M) == 0
        assert _linear_fwd_status(None, 3, 0, 100, 7, True, M=M, N=100, n_store=0) == 0


def _wgrad_status(P, det=False, **over):
    a = dict(Z=P, ldz=_GEMM_N, X=P, ldx=128, dW=P, ldw=128, zeros=P, M=_GEMM_M, N=_GEMM_N, K=128, n_valid=_GEMM_N, k_valid=128, dtype=1, variant=0,
             ws=P, ws_floats=1 << 40, stream=None)
    a.update(over)
    if a["ws_floats"] == "short":
        a["ws_floats"] = _lib.query("snerf_linear_wgrad_ws_floats", a["M"], a["N"], a["K"], a["ldz"], a["ldx"], a["dtype"], a["variant"]) - 1
    name = "snerf_linear_wgrad_det" if det else "snerf_linear_wgrad"
    return getattr(_lib.load(), name)(*[a[arg] for _, arg in _lib.parse_header()[name]])


def test_linear_wgrad_keeps_its_refusals():
    """snerf_linear_wgrad / snerf_linear_wgrad_det: every refusal of the weight-gradient host path, through both entries where both have it"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    # refusals and empty batches only: nothing is launched.  Where there is a GPU the pointers are still a device allocation that covers the
    # largest case (the 8192 x 1024 16-bit operands: 16 MiB; the 64 MiB of partial tiles of the 1024-wide plans), so that a regression which
    # accepts one of them runs on real memory
    P, keep = _gemm_ptr(80)
    both = {"no kernels for fp64": dict(dtype=3), "no kernels for fp16 + fp8": dict(dtype=5),
            "split-bf16: N % 128": dict(dtype=4, N=192, ldz=192, n_valid=96), "split-bf16: K % 128": dict(dtype=4, K=192, ldx=192, k_valid=96),
            "hi half of a split activation: fp32": dict(dtype=0, variant=1 << 14), "hi half of a split activation: split operands": dict(dtype=4, variant=1 << 14),
            "N % 8": dict(N=260, ldz=264), "K % 8": dict(K=132, ldx=136), "ldz % 8": dict(ldz=260), "ldx % 8": dict(ldx=132),
            "N % 4 (fp32)": dict(dtype=0, N=258, ldz=260), "K % 4 (fp32)": dict(dtype=0, K=130, ldx=132), "ldz % 4 (fp32)": dict(dtype=0, ldz=258),
            "ldx % 4 (fp32)": dict(dtype=0, ldx=130), "N below a vector": dict(N=0), "K below a vector": dict(K=4), "no zero page": dict(zeros=None, M=320)}      # (whole 32-row stages: no row would be read from it)
    for what, change in both.items():
        for det in (False, True):
            assert _wgrad_status(P, det, **change) == 1, (what, det)
    assert _wgrad_status(P, True, dtype=4, N=256, K=128) == 1        # the split-bf16 operands have no deterministic fold
    assert _wgrad_status(P, True, ws=None) == 1 and _wgrad_status(P, True, ws=None, M=0) == 1
    for dt, variant in ((0, 0), (1, 0), (1, 2), (2, 3), (1, 128)):
        assert _wgrad_status(P, True, dtype=dt, variant=variant, ws_floats="short") == 1, (dt, variant)
    for M in (4096, 8192):                                            # the 1024-wide layer: 128 x 128 tiles below 512 rows per slice, 256 x 256 from there
        assert _wgrad_status(P, True, M=M, N=1024, K=1024, ldz=1024, ldx=1024, n_valid=1024, k_valid=1024, ldw=1024, variant=2, ws_floats="short") == 1, M
    for M in (0, -1):
        assert _wgrad_status(None, False, M=M, dtype=3, N=1, K=1) == 0 and _wgrad_status(P, True, M=M, dtype=3, ws_floats=0) == 0
    if keep is not None:
        import torch
        torch.cuda.synchronize()


def test_linear_wgrad_workspace_query_pins_the_plan():
    """snerf_linear_wgrad_ws_floats = slices x floats per slice of the launch plan (tn_plan), on both sides of each of its rules, at the 256 CUs
    of an MI355X (also what the library assumes without a device): the 256 x 256 kernel (variant bit 1) from M = 4096 and from eight k-tiles per
    slice up to M = 131072, the 128 x 128 kernel's 256-row floor below that.  ld = width, bf16."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    q = lambda M, N, K, variant: _lib.query("snerf_linear_wgrad_ws_floats", M, N, K, N, K, _BF16, variant)
    for (M, N, K), expect in {(4096, 1024, 1024): (16777216, 16777216), (512, 1024, 1024): (2097152, 2097152), (32768, 256, 256): (8388608, 8388608),
                              (700, 64, 128): (49152, 49152), (70001, 1024, 1152): (17694720, 15728640)}.items():
        assert (q(M, N, K, 0), q(M, N, K, 3)) == expect, (M, N, K)
    assert q(0, 256, 256, 0) == 0 and q(256, 0, 256, 0) == 0 and q(256, 256, -1, 3) == 0
    assert _lib.query("snerf_linear_wgrad_ws_floats", 70001, 1024, 1152, 1024, 1152, _F16, 3) == 15728640      # fp16 runs the bf16 plan


# ---- the host statuses of the hash-grid entries (csrc/zip.hip) --------------------------------------------------------------------------------
_ZC = (1, 2, 3, 4, 8)
_ZIP_SELF_CONTAINED = ("snerf_zip_encode_fwd", "snerf_zip_encode_prop_fwd", "snerf_zip_prop_mlp_fwd", "snerf_zip_prop_mlp_bwd", "snerf_zip_encode_fwd_count",
                       "snerf_zip_encode_bwd", "snerf_zip_encode_ray_bwd", "snerf_zip_bin_scale")
# Per entry: the axes of its dtype / channel / flavour arguments and, over their full cross product (last axis fastest), `x` = refused
# ("bad argument"), `.` = reaches a launch.  Read off the library before the entries' type ladders were folded into one dispatch.
_ZIP_CROSS = {
    "snerf_zip_encode_fwd": (dict(table_dtype=range(4), feat_dtype=range(4), C=_ZC),
                             "..x.. ..x.. ..x.. xxxxx  xxxxx xxxxx xxxxx xxxxx  ..x.. ..x.. ..x.. xxxxx  xxxxx xxxxx xxxxx xxxxx"),
    "snerf_zip_encode_prop_fwd": (dict(table_dtype=range(4)), ".x.x"),
    "snerf_zip_prop_mlp_fwd": (dict(feat_dtype=range(4), round_bf16=range(4), L=(2, 12)), "....xxxx ....xxxx xxxx..xx xxxxxxxx"),
    "snerf_zip_prop_mlp_bwd": (dict(feat_dtype=range(4), round_bf16=range(4), L=(2, 12)), "....xxxx ....xxxx xxxx..xx xxxxxxxx"),
    "snerf_zip_encode_fwd_count": (dict(table_dtype=range(4), feat_dtype=range(4), C=_ZC),
                                   ".xx.x .xx.x .xx.x xxxxx  xxxxx xxxxx xxxxx xxxxx  .xx.x .xx.x .xx.x xxxxx  xxxxx xxxxx xxxxx xxxxx"),
    "snerf_zip_encode_bwd": (dict(feat_dtype=range(4), C=_ZC, lds_levels=(0, 1)), "....xx.... ....xx.... ....xx.... xxxxxxxxxx"),
    "snerf_zip_encode_ray_bwd": (dict(table_dtype=range(4), feat_dtype=range(4), C=_ZC),
                                 ".xx.x .xx.x .xx.x xxxxx  xxxxx xxxxx xxxxx xxxxx  .xx.x .xx.x .xx.x xxxxx  xxxxx xxxxx xxxxx xxxxx"),
    "snerf_zip_bin_scale": (dict(feat_dtype=range(4)), "...x"),
    # (passes -1 .. 10 per channel count; the accumulate passes 2 and 7 never look at the gradient's dtype)
    "snerf_zip_encode_bwd_binned": (dict(feat_dtype=range(4), C=_ZC, **{"pass": range(-1, 11)}),
                                    "x..........x xxxxxxxxxxxx xxxxxxxxxxxx x..........x xxxxxxxxxxxx " * 3
                                    + "xxx.xxxx.xxx xxxxxxxxxxxx xxxxxxxxxxxx xxx.xxxx.xxx xxxxxxxxxxxx"),
    # (gradient fp32 / fp16 x table gradient fp32 / fp16; half records asked for at C = 2 / 8 are fp32 records, not a refusal)
    "snerf_grid_encode_bwd_binned": (dict(grad_dtype=range(4), out_dtype=range(4), C=_ZC, half_records=(0, 1)),
                                     ("....xx.... xxxxxxxxxx ....xx.... xxxxxxxxxx " + "x" * 40) * 2),
}
# snerf_zip_encode_bwd_binned, pass -1 .. 10 (columns) with one pointer absent (rows; the first row: none absent), C = 4, bf16 gradients
_ZIP_PASS_PTRS = ("grad_feat", "grad_table", "ksplit_host", "level_rows_host", "counts", "wg_offsets", "starts", "rec_row", "rec_val", "scale_exp")
_ZIP_PASSES = """x..........x xxx.xxxx.xxx x..x....x..x xxxxxxxxxxxx xxxxxxxxxxxx xxxxxxxxxxxx xxx.xxxx.xxx x.xxxxxxxxxx x.xxxxxxxxxx x.xxxxxxxxxx
                 x..x..xxx.xx"""


def _zip_problem():
    """Real operands of one tiny problem for every hash-grid entry: R = 4 rays x S = 2 intervals, L = 2 levels (one dense, one hashed; the
    layout of ops.grid_level_layout), n = 7 multisamples, every buffer sized for the widest case of the lists (C = 8, 4-byte elements), on the
    device where there is one -- an accepted case then runs on valid memory -- and on the host otherwise (no launch happens there).  The
    `*_host` arrays are numpy: the library reads them on the host.  -> ({argument name: value}, what must stay alive)"""
    import numpy as np
    import torch
    from snerf_amd import ops
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    R, S, L, n, B = 4, 2, 2, 7, 8
    g = torch.Generator().manual_seed(12)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    unit = lambda t: torch.nn.functional.normalize(t, dim=-1)
    off, sizes = ops.grid_level_layout(3, L, 2.0, 16, 12)               # 17^3 -> 4920 rows (dense), 33^3 -> 4096 rows (hashed)
    rows = int(off[-1])
    d = unit(rnd(R, 3))
    bx = unit(torch.cross(d, rnd(R, 3), dim=-1))
    t = dict(tdist=torch.sort(torch.rand(R, S + 1, generator=g) * 5 + 0.2, -1)[0], origins=rnd(R, 3) * 0.1, directions=d,
             radii=2e-3 + 2e-3 * torch.rand(R, generator=g), base_x=bx, base_y=unit(torch.cross(d, bx, dim=-1)),
             deg_jitter=torch.rand(R, S, n, generator=g), table=rnd(rows, 8) * 0.1, offsets=torch.from_numpy(off), grid_sizes=torch.from_numpy(sizes),
             feat=torch.zeros(R * S, 16), grad_feat=rnd(R * S, 16) * 1e-3, grad_table=torch.zeros(rows, 8), grad_table_bf16=torch.zeros(rows, 8),
             w1=rnd(8, 16) * 0.3, b1=rnd(8) * 0.1, w2=rnd(8) * 0.3, b2=rnd(1), raw_density=torch.zeros(R * S), raw=torch.zeros(R * S),
             F=rnd(R * S, 16) * 0.5, d_raw=rnd(R * S) * 1e-3, dF=torch.zeros(R * S, 16), g_w1=torch.zeros(8, 16), g_b1=torch.zeros(8), g_w2=torch.zeros(8),
             g_b2=torch.zeros(1), counts=torch.zeros(L, 1024, dtype=torch.int32), wg_offsets=torch.zeros(L, 1024, dtype=torch.int32),
             starts=torch.zeros(L, 1024, dtype=torch.int64), rec_row=torch.zeros(4096, dtype=torch.int16), rec_val=torch.zeros(4096, 8),
             g64=torch.zeros(rows, 8, dtype=torch.int64), scale_exp=torch.zeros(2, dtype=torch.int32), g_origins=torch.zeros(R, 3),
             g_directions=torch.zeros(R, 3), g_base_x=torch.zeros(R, 3), g_base_y=torch.zeros(R, 3), grad=rnd(B, L * 8) * 1e-3,
             inputs=torch.rand(B, 3, generator=g), grad_embeddings=torch.zeros(rows, 8))
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    host = dict(ksplit_host=np.ones(L, dtype=np.int32), level_rows_host=np.diff(off).astype(np.int32), offsets_host=np.ascontiguousarray(off))
    ws_bytes = max(_lib.query("snerf_grid_encode_bwd_binned_ws_bytes", B, C, L, host["offsets_host"].ctypes.data, 0) for C in (1, 2, 4, 8))
    t["ws"] = torch.zeros(ws_bytes + 256, dtype=torch.uint8, device=dev)
    a = {k: v.data_ptr() for k, v in t.items()}
    a.update({k: v.ctypes.data for k, v in host.items()})
    a["ws"] = (a["ws"] + 255) & ~255                                    # (the stand-alone encoder's workspace must be 256-byte aligned)
    a.update(R=R, S=S, L=L, n=n, m=3, Sl=1.0, H=16, std_scale=0.35, C=4, ld=16, table_dtype=_F32, feat_dtype=_BF16, levels_per_thread=0, hidden=8,
             round_bf16=1, P=R * S, ldf=16, lddf=16, ws_floats=_lib.query("snerf_zip_prop_mlp_ws_floats", 12, 8, R * S), lds_levels=0, lds_cells=0,
             lds_slabs=0, rows=R * S, cols=4, capacity=4096, g64_rows=0, B=B, grad_dtype=_F32, out_dtype=_F32, half_records=0, ws_bytes=ws_bytes,
             stream=None)
    a["pass"] = 0
    a["grad_table_bf16"], a["bf16_image"] = None, a["grad_table_bf16"]  # (optional: absent unless a case asks for it)
    return a, (t, host)


def _zip_status(name, a, **over):
    v = dict(a, **over)
    if name == "snerf_grid_encode_bwd_binned":                         # (its S is the levels' log2 growth; the gradient is point-major [B, L C])
        v["S"] = 1.0
        v.setdefault("grad_stride_l", v["C"])
        v.setdefault("grad_stride_b", v["L"] * v["C"])
    if v["lds_levels"] == 1 and "lds_cells" not in over:               # level 0 (4920 rows) as one LDS slab: 4920 C floats <= 160 KiB up to C = 8
        v.update(lds_cells=4920, lds_slabs=1)
    return getattr(_lib.load(), name)(*[v[arg] for _, arg in _lib.parse_header()[name]])


def _zip_rows_host(*rows):
    import numpy as np
    return np.array(rows, dtype=np.int32)


def _zip_refusals(a):
    """every single-argument refusal of each entry: {entry: [change, ...]} against the accepted base case (C = 4, fp32 table, bf16 features)"""
    big, zero, k0 = _zip_rows_host(4913, 1 << 23), _zip_rows_host(4920, 0), _zip_rows_host(1, 0)     # 2^23 rows at C = 4: 2048 row ranges
    per_level = [dict(level_rows_host=big.ctypes.data), dict(level_rows_host=zero.ctypes.data), dict(ksplit_host=k0.ctypes.data)]
    mlp = [dict(L=0), dict(L=17), dict(ldf=1), dict(hidden=0), dict(hidden=65)] + _nulls("F", "w1", "b1", "w2", "b2")
    off_empty, off_big = _zip_rows_host(0, 4920, 4920), _zip_rows_host(0, 8, 8 + (1 << 23))
    return (big, zero, k0, off_empty, off_big), {
        "snerf_zip_encode_fwd": [dict(S=0), dict(L=0), dict(n=0), dict(ld=7), dict(levels_per_thread=-1)] + _nulls("table", "feat", "grid_sizes"),
        "snerf_zip_encode_prop_fwd": [dict(S=0), dict(L=0), dict(L=17), dict(n=0), dict(n=9), dict(hidden=0), dict(hidden=1025)]
                                     + _nulls("table", "grid_sizes", "w1", "b1", "w2", "b2", "raw_density"),
        "snerf_zip_prop_mlp_fwd": mlp + _nulls("raw"),
        "snerf_zip_prop_mlp_bwd": mlp + [dict(lddf=1), dict(lddf=65), dict(ws_floats=a["ws_floats"] - 1, L=12)]
                                  + _nulls("d_raw", "dF", "g_w1", "g_b1", "g_w2", "g_b2", "ws"),
        "snerf_zip_encode_fwd_count": [dict(S=0), dict(L=0), dict(L=17), dict(n=0), dict(n=9), dict(ld=7)] + per_level
                                      + _nulls("table", "feat", "grid_sizes", "ksplit_host", "level_rows_host", "counts", "wg_offsets"),
        "snerf_zip_encode_bwd": [dict(S=0), dict(L=0), dict(n=0), dict(ld=7), dict(grad_table_bf16=a["bf16_image"] + 2), dict(grad_table_bf16=a["bf16_image"], C=3),
                                 dict(lds_levels=-1), dict(lds_levels=3), dict(lds_levels=1, lds_cells=0, lds_slabs=1),
                                 dict(lds_levels=1, lds_cells=10241, lds_slabs=1), dict(lds_levels=1, lds_cells=4920, lds_slabs=0)]
                                + _nulls("grad_feat", "grad_table", "grid_sizes"),
        "snerf_zip_encode_bwd_binned": [dict(S=0), dict(L=0), dict(L=17), dict(n=0)] + per_level + _nulls("ksplit_host", "level_rows_host", "counts"),
        "snerf_zip_encode_ray_bwd": [dict(S=0), dict(L=0), dict(n=0)] + _nulls("table", "grad_feat", "g_origins", "g_directions", "g_base_x", "g_base_y"),
        "snerf_zip_bin_scale": [dict(cols=0), dict(ld=3)] + _nulls("scale_exp", "grad_feat"),
        "snerf_grid_encode_bwd_binned": [dict(L=0), dict(L=17), dict(ws=a["ws"] + 128), dict(ws_bytes=0), dict(ws_bytes=256), dict(grad_stride_l=5),
                                         dict(grad_stride_b=9), dict(offsets_host=off_empty.ctypes.data), dict(offsets_host=off_big.ctypes.data)]
                                        + _nulls("grad", "inputs", "offsets", "offsets_host", "grad_embeddings", "ws"),
    }


@pytest.mark.parametrize("entry", sorted(_ZIP_CROSS))
def test_hash_grid_entries_keep_their_statuses(entry):
    """Every hash-grid entry whose host code dispatches on a dtype or a channel count: the full cross product of those arguments is refused
    exactly where recorded, each single-argument refusal it has is "bad argument", and an empty batch is OK before anything is looked at.
    What is not refused reaches a launch: "launch failed" without a device.  With one, the self-contained entries launch every accepted case
    on the real operands of _zip_problem and must return OK (a wrongly routed instantiation shows as a status, not as a fault); the two
    multi-pass entries (their later passes read what earlier ones wrote) run only their refusals and empty batches there -- the value tests
    of test_zip_paths.py and test_gpu_grid.py reach their accepted cases in order."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    import itertools
    import torch
    a, keep = _zip_problem()
    gpu = torch.cuda.is_available()
    launch = gpu and entry in _ZIP_SELF_CONTAINED
    accepted = lambda rc: rc == (0 if launch else 2)
    axes, marks = _ZIP_CROSS[entry]
    marks = marks.replace(" ", "")
    combos = list(itertools.product(*axes.values()))
    assert len(marks) == len(combos)
    for combo, mark in zip(combos, marks):
        case = dict(zip(axes, combo))
        if mark == "x":
            assert _zip_status(entry, a, **case) == 1, (entry, case)
        elif launch or not gpu:
            rc = _zip_status(entry, a, **case)
            assert accepted(rc), (entry, case, rc)
    keep2, refusals = _zip_refusals(a)
    for change in refusals[entry]:
        assert _zip_status(entry, a, **change) == 1, (entry, change)
    if entry == "snerf_zip_encode_bwd_binned":
        rows = _ZIP_PASSES.split()
        assert len(rows) == 1 + len(_ZIP_PASS_PTRS)
        for absent, row in zip((None,) + _ZIP_PASS_PTRS, rows):
            for p, mark in zip(range(-1, 11), row):
                if mark == "x" or not gpu:
                    rc = _zip_status(entry, a, **{"pass": p}, **({absent: None} if absent else {}))
                    assert rc == (1 if mark == "x" else 2), (absent, p, rc)
    batch = {"snerf_zip_prop_mlp_fwd": "P", "snerf_zip_prop_mlp_bwd": "P", "snerf_grid_encode_bwd_binned": "B", "snerf_zip_bin_scale": None}.get(entry, "R")
    if batch is None:                                                   # snerf_zip_bin_scale: no rows is a launch of its own (the default scale)
        assert accepted(_zip_status(entry, a, rows=0, grad_feat=None, cols=0, feat_dtype=3))
    else:
        nothing = dict(a, **{arg: None for ty, arg in _lib.parse_header()[entry] if ty is ctypes.c_void_p})          # (no pointer at all)
        for empty in (0, -1):
            assert _zip_status(entry, a, **{batch: empty}) == 0
            assert _zip_status(entry, dict(nothing, C=3, L=99, n=-1, table_dtype=3, feat_dtype=3, grad_dtype=3, **{"pass": 11}), **{batch: empty}) == 0
    if gpu:
        torch.cuda.synchronize()
    del keep, keep2
