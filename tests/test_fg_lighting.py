"""The lighting match of S-NeRF++ stage 1 (s-nerfpp/stage1_code/utils_render.py:1008-1051 handle_lighting): the numpy model in
snerf_amd/foreground.py against documented and hand-computed answers, and on the GPU snerf_fg_hsv / snerf_fg_lighting and
composite_frame(lighting=) bit for bit against that model.

PARITY UNPINNED: cv2 is not installed where this was written, so the two 8-bit conversions are restated from OpenCV's published scalar
code (imgproc color_hsv) and no vector from the library itself exists; the round-trip figures below pin the restatement against an
accidental edit, not against cv2.  Everything after the conversions is the reference's own numpy."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import foreground as of
from snerf_amd import _lib
from snerf_amd import foreground as fgm

gpu = pytest.mark.gpu

ANCHORS = (((255, 0, 0), (0, 255, 255)), ((0, 255, 0), (60, 255, 255)), ((0, 0, 255), (120, 255, 255)), ((255, 255, 0), (30, 255, 255)),
           ((0, 255, 255), (90, 255, 255)), ((255, 0, 255), (150, 255, 255)), ((255, 255, 255), (0, 0, 255)), ((128, 128, 128), (0, 0, 128)),
           ((10, 20, 30), (105, 170, 30)))


@functools.lru_cache(maxsize=None)
def _all_triples():
    """every 8-bit triple once, [4096,4096,3] (byte 0 fastest), and its two conversions by the host model; computed once, never written to"""
    i = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([i & 255, (i >> 8) & 255, i >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    out = px, fgm.rgb_to_hsv_u8_host(px), fgm.hsv_to_rgb_u8_host(px)
    for a in out:
        a.setflags(write=False)
    return out


def test_rgb_to_hsv_anchors_and_back():
    """OpenCV's documented 8-bit values (H = degrees / 2, S and V scaled to 255) of the primaries, secondaries and greys, and
    (10, 20, 30) by hand: v = 30, diff = 20, s = (20 * 34816 + 2048) >> 12 = 170, h = ((10 - 20 + 80) * 6144 + 2048) >> 12 = 105"""
    for rgb, hsv in ANCHORS:
        got = fgm.rgb_to_hsv_u8_host(np.array(rgb, np.uint8))
        assert got.dtype == np.uint8 and tuple(int(v) for v in got) == hsv, (rgb, got)
        back = fgm.hsv_to_rgb_u8_host(got)
        assert back.dtype == np.uint8 and tuple(int(v) for v in back) == rgb, (rgb, back)
    px = np.array([a[0] for a in ANCHORS], np.uint8).reshape(3, 3, 3)
    assert np.array_equal(fgm.rgb_to_hsv_u8(px), np.array([a[1] for a in ANCHORS], np.uint8).reshape(3, 3, 3))      # numpy in: the host model
    assert np.array_equal(fgm.hsv_to_rgb_u8(fgm.rgb_to_hsv_u8(px)), px)


def test_hsv_round_trip_over_all_triples():
    """hsv2rgb(rgb2hsv(.)) over all 2^24 triples: the largest channel error is 5 and 68.9 % of the triples change -- what this
    restatement gives (it pins the model against an edit, not against cv2)"""
    px, hsv, _ = _all_triples()
    assert int(hsv[..., 0].max()) == 179
    back = fgm.hsv_to_rgb_u8_host(hsv)
    err = np.abs(back.astype(np.int16) - px.astype(np.int16))
    share = float((err.max(axis=-1) > 0).mean())
    print("largest channel error", int(err.max()), "changed share", share)
    assert int(err.max()) == 5
    assert abs(share - 0.689) <= 0.001, share
    grey = px[(px[..., 0] == px[..., 1]) & (px[..., 1] == px[..., 2])]
    assert np.array_equal(fgm.hsv_to_rgb_u8_host(fgm.rgb_to_hsv_u8_host(grey)), grey)        # s = 0: greys come back unchanged


def _tiny():
    """the frame of test_lighting_by_hand: grey pixels (r = g = b = V), which the round trip leaves unchanged"""
    V = np.array([[255, 0, 255, 190, 10, 200],
                  [0, 255, 0, 210, 100, 250],
                  [255, 0, 255, 195, 205, 203],
                  [0, 255, 0, 255, 0, 255]], np.uint8)
    im = V[..., None].repeat(3, -1)
    mask = np.zeros((4, 6, 3), np.uint8)
    mask[0, 4] = (1, 0, 0)                  # a 1 in channel 0 alone is foreground
    mask[1, 4] = (255, 255, 255)
    mask[1, 5] = (255, 0, 0)
    mask[2, 4] = (0, 255, 255)              # channel 0 zero: background, whatever channels 1 and 2 hold
    mask[3, 0] = (0, 7, 0)
    return im, mask


def test_lighting_by_hand():
    """4 x 6, grey pixels.  fg = {(0,4), (1,4), (1,5)} with V = 10, 100, 250: n_fg = 3, sum = 360, sum of squares = 100 + 10000 + 62500 =
    72600, fg_mean = 120.  Raw box rows 0..1, cols 4..5, lengths 1 and 1, so it grows by 1 // 2 + 1 = 1 per side: rows [max(0, -1),
    min(3, 2)] = [0, 2] (clamped at the top), cols [max(0, 3), min(5, 6)] = [3, 5] (clamped at the right).  bg = the six other pixels
    of that 3 x 3 box, (2,4) with mask (0, 255, 255) among them: V = 190, 210, 195, 205, 203, 200, sum 1203, bg_mean = 200.5.  The
    columns 0..2 and row 3 hold 0 / 255 and are outside the box.  V' = trunc(clip(V - 120 + 200.5, 0, 255)): 10 -> 90.5 -> 90,
    100 -> 180.5 -> 180, 250 -> 330.5 -> 255 (clipped).  Greys stay greys, every other pixel comes back unchanged."""
    im, mask = _tiny()
    assert fgm.lighting_stats_host(im, mask).tolist() == [0, 1, 4, 5, 3, 360, 72600, 6, 1203]
    want = im.copy()
    want[0, 4], want[1, 4], want[1, 5] = 90, 180, 255
    before = im.copy()
    got = fgm.handle_lighting_host(im, mask)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(im, before) and got is not im                                        # a new array
    assert np.array_equal(fgm.handle_lighting(im, mask), want)                                 # the reference's own call, on numpy arrays
    # a shift of less than one level leaves every V where it was: fg 255, 254, 90 (mean 599 / 3), V' = trunc(V - 199.67 + 200.5)
    im2 = im.copy()
    im2[0, 4], im2[1, 4], im2[1, 5] = 255, 254, 90
    assert np.array_equal(fgm.handle_lighting_host(im2, mask), im2)
    # a downward shift: every V >= 190 lowered by 180 -> bg 10, 30, 15, 25, 23, 20 (mean 20.5), fg 75, 74, 90 (mean 239 / 3)
    im2[im2 >= 190] -= 180
    want2 = im2.copy()
    want2[0, 4], want2[1, 4], want2[1, 5] = 15, 14, 30                                          # 75 - 79.67 + 20.5 = 15.83, then 14.83, 30.83
    assert np.array_equal(fgm.handle_lighting_host(im2, mask), want2)
    # a shift that clips at 0: fg 10, 250, 250 and every V >= 190 lowered by 190 -> bg 0, 20, 5, 15, 13, 10 (mean 10.5), fg 10, 60, 60 (mean 130 / 3)
    im3 = im.copy()
    im3[0, 4], im3[1, 4], im3[1, 5] = 10, 250, 250
    im3[im3 >= 190] -= 190
    want3 = im3.copy()
    want3[0, 4], want3[1, 4], want3[1, 5] = 0, 27, 27                                           # 10 - 43.33 + 10.5 = -22.83 -> 0 (clipped); 60 -> 27.17
    assert np.array_equal(fgm.handle_lighting_host(im3, mask), want3)


def _blob(H, W, cy, cx, ry, rx, value=(255, 255, 255)):
    yy, xx = np.mgrid[:H, :W]
    m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return m[..., None] * np.array(value, np.uint8)


def _round_trip(im):
    return fgm.hsv_to_rgb_u8_host(fgm.rgb_to_hsv_u8_host(im))


def _cases(H=37, W=53):
    """name -> (frame, mask) at H x W: every branch of handle_lighting"""
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    cases = {}
    cases["interior"] = frame, _blob(H, W, 18, 25, 7, 11)
    cases["top_right"] = frame, _blob(H, W, 2, 49, 8, 9)
    single = np.zeros((H, W, 3), np.uint8); single[20, 31] = 255
    cases["single_pixel"] = frame, single
    cases["empty"] = frame, np.zeros((H, W, 3), np.uint8)
    cases["full_frame"] = frame, np.full((H, W, 3), 255, np.uint8)
    m = _blob(H, W, 18, 25, 7, 11)
    const = frame.copy()
    const[m[..., 0] > 0] = np.minimum(const[m[..., 0] > 0], 77)
    const[..., 1][m[..., 0] > 0] = 77                                                        # max(r, g, b) = 77 on every fg pixel
    cases["constant_v"] = const, m
    bright = (frame // 8).astype(np.uint8)                                                   # surround V <= 31
    bright[m[..., 0] > 0] = rng.integers(150, 256, (int((m[..., 0] > 0).sum()), 3)).astype(np.uint8)
    cases["bright_on_dark"] = bright, m
    dark = (255 - frame // 8).astype(np.uint8)                                               # surround V >= 224
    dark[m[..., 0] > 0] = rng.integers(0, 120, (int((m[..., 0] > 0).sum()), 3)).astype(np.uint8)
    cases["dark_on_bright"] = dark, m
    ch0 = _blob(H, W, 18, 25, 7, 11, (1, 0, 0))                                              # a 1 in channel 0 alone is fg
    ch0 = ch0 + _blob(H, W, 18, 40, 5, 3, (0, 255, 255)) * (ch0[..., :1] == 0)               # channel 0 zero, channels 1 / 2 set: bg, inside the box
    cases["channel0"] = frame, ch0.astype(np.uint8)
    return cases


def test_lighting_degenerate_cases_and_keep_background():
    cases = _cases()
    for name in ("empty", "constant_v", "full_frame"):                                       # full_frame: the documented deviation (n_bg = 0)
        im, mask = cases[name]
        assert np.array_equal(fgm.handle_lighting_host(im, mask), _round_trip(im)), name
    assert fgm.lighting_stats_host(*cases["empty"]).tolist() == [37, -1, 53, -1, 0, 0, 0, 0, 0]
    s = fgm.lighting_stats_host(*cases["full_frame"])
    assert s[:5].tolist() == [0, 36, 0, 52, 37 * 53] and s[7:].tolist() == [0, 0]
    s = fgm.lighting_stats_host(*cases["constant_v"])
    assert s[5] == 77 * s[4] and s[6] == 77 * 77 * s[4] and s[7] > 0
    # n_bg counts the expanded box alone: a band over all columns and rows 0 .. 3 grows to rows 0 .. 5 and finds its bg in rows 4 and 5
    im = cases["interior"][0]
    band = np.zeros_like(im); band[:4] = 255
    assert fgm.lighting_stats_host(im, band)[7] > 0
    band[:] = 255
    assert fgm.lighting_stats_host(im, band)[7] == 0
    for name in ("interior", "top_right", "single_pixel", "bright_on_dark", "channel0", "empty"):
        im, mask = cases[name]
        full, kept = fgm.handle_lighting_host(im, mask), fgm.handle_lighting_host(im, mask, keep_background=True)
        fg = mask[..., 0] > 0
        assert np.array_equal(kept[~fg], im[~fg]) and np.array_equal(kept[fg], full[fg]), name
        if name in ("empty", "single_pixel"):                                                # one pixel has no variance: the box (8 bg pixels) is found, V stays
            assert np.array_equal(full, _round_trip(im)), name
        else:
            assert not np.array_equal(full, _round_trip(im)), name                           # the shift does something
    assert fgm.lighting_stats_host(*cases["single_pixel"])[[0, 1, 2, 3, 4, 7]].tolist() == [20, 20, 31, 31, 1, 8]
    im, mask = cases["channel0"]
    s = fgm.lighting_stats_host(im, mask)
    only0 = np.where(mask[..., :1] > 0, 255, 0).astype(np.uint8).repeat(3, -1)               # what channel 0 alone says
    assert np.array_equal(s, fgm.lighting_stats_host(im, only0)) and s[4] == int((mask[..., 0] == 1).sum()) > 0
    assert np.array_equal(fgm.handle_lighting_host(im, mask), fgm.handle_lighting_host(im, only0))
    assert ((mask[..., 0] == 0) & (mask[..., 1] == 255)).any()


def test_bad_arguments_are_rejected_without_a_gpu():
    """validation happens before any launch: both entries return 1 for each bad argument, with no device.  The non-null pointers are
    host addresses nobody reads."""
    buf = ctypes.create_string_buffer(128)
    p = ctypes.addressof(buf)
    bad_hsv = ((None, 4, 0), (p, 0, 0), (p, -3, 1), (p, 4, 2), (p, 4, -1))
    for args in bad_hsv:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_fg_hsv", *args, None)
    bad_light = ((None, p, 4, 4, 0, p), (p, None, 4, 4, 0, p), (p, p, 4, 4, 0, None), (p, p, 0, 4, 0, p), (p, p, 4, 0, 0, p), (p, p, -1, 4, 1, p),
                 (p, p, 4096, 2049, 0, p), (p, p, (1 << 23) + 1, 1, 0, p), (p, p, 65536, 65536, 0, p), (p, p, 4, 4, 2, p), (p, p, 4, 4, -1, p))
    for args in bad_light:
        with pytest.raises(_lib.SnerfHipError, match="bad argument"):
            _lib.call("snerf_fg_lighting", *args, None)


def test_composite_frame_refuses_an_unknown_lighting_mode():
    with pytest.raises(ValueError, match="lighting"):
        fgm.composite_frame(None, None, None, [], lighting="x")


# ---- on the GPU: bit for bit against the host model ------------------------------------------------------------------------------------
def _c(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@gpu
@pytest.mark.parametrize("to_rgb", (0, 1))
def test_fg_hsv_all_triples(to_rgb):
    """all 2^24 input triples in one [4096,4096,3] tensor per direction; for to_rgb = 1 that includes H >= 180"""
    px, hsv, rgb = _all_triples()
    t = _c(px.copy())
    got = (fgm.hsv_to_rgb_u8 if to_rgb else fgm.rgb_to_hsv_u8)(t)
    assert got is t
    assert np.array_equal(t.cpu().numpy(), rgb if to_rgb else hsv)


@gpu
def test_fg_hsv_small_counts_and_unaligned_views():
    """P in {1, 3, 5, 4099} (head, tail and word paths, more than one workgroup), at the start of a buffer and as a view that starts 3
    bytes (one pixel) -- and 1 and 2 bytes -- into one; the bytes around the view stay as they were"""
    rng = np.random.default_rng(5)
    for P in (1, 3, 5, 4099):
        src = rng.integers(0, 256, (P, 3)).astype(np.uint8)
        for to_rgb, fn, ref in ((0, fgm.rgb_to_hsv_u8, fgm.rgb_to_hsv_u8_host), (1, fgm.hsv_to_rgb_u8, fgm.hsv_to_rgb_u8_host)):
            want = ref(src)
            for lead in (0, 3, 1, 2):
                buf = torch.full((lead + 3 * P + 5,), 0xA5, dtype=torch.uint8, device="cuda")
                view = buf[lead:lead + 3 * P].view(P, 3)
                view.copy_(_c(src))
                fn(view)
                out = buf.cpu().numpy()
                assert np.array_equal(out[lead:lead + 3 * P].reshape(P, 3), want), (P, to_rgb, lead)
                assert (out[:lead] == 0xA5).all() and (out[lead + 3 * P:] == 0xA5).all(), (P, to_rgb, lead)


@gpu
def test_fg_lighting_small_frames_vs_host_model():
    """37 x 53 (odd, no multiple of the four pixels of a lane, two workgroups in the apply pass): image and stats against the host model for every branch"""
    cases = _cases()
    for name, (lo, hi) in (("bright_on_dark", (True, False)), ("dark_on_bright", (False, True))):      # conditions on the fixture: both clip branches run
        im, mask = cases[name]
        s = fgm.lighting_stats_host(im, mask).astype(np.float64)
        fg = mask[..., 0] > 0
        pre = im.max(axis=-1)[fg] - s[5] / s[4] + s[8] / s[7]
        out_v = fgm.handle_lighting_host(im, mask).max(axis=-1)[fg]
        assert bool((pre < 0).any()) == lo and bool((pre > 255).any()) == hi, name
        assert (out_v[pre < 0] == 0).all() and (out_v[pre > 255] == 255).all(), name
    for name, (im, mask) in cases.items():
        for keep in (False, True):
            want, want_stats = fgm.handle_lighting_host(im, mask, keep), fgm.lighting_stats_host(im, mask)
            t, stats = _c(im), torch.full((9,), -7, dtype=torch.int64, device="cuda")
            assert fgm.handle_lighting(t, _c(mask), keep_background=keep, stats=stats) is t
            assert np.array_equal(stats.cpu().numpy(), want_stats), (name, keep, stats.cpu().numpy(), want_stats)
            assert np.array_equal(t.cpu().numpy(), want), (name, keep)
    # frame and mask at different byte offsets: the mask goes through the byte path
    im, mask = cases["top_right"]
    for lead_im, lead_mask in ((1, 0), (0, 2), (3, 3)):
        bi = torch.zeros(lead_im + im.size, dtype=torch.uint8, device="cuda")
        bm = torch.zeros(lead_mask + mask.size, dtype=torch.uint8, device="cuda")
        vi, vm = bi[lead_im:].view(im.shape), bm[lead_mask:].view(mask.shape)
        vi.copy_(_c(im)); vm.copy_(_c(mask))
        fgm.handle_lighting(vi, vm)
        assert np.array_equal(vi.cpu().numpy(), fgm.handle_lighting_host(im, mask)), (lead_im, lead_mask)


@gpu
def test_fg_lighting_full_size_frame_two_instances():
    """1280 x 1920, two blobs, one crossing the right border: two calls in a row against the host model called twice; the same on a
    fresh copy gives the same bytes (integer sums: no dependence on the order of the atomics)"""
    H, W = 1280, 1920
    rng = np.random.default_rng(12)
    im = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    im[500:1000] //= 3
    masks = [_blob(H, W, 700, 500, 260, 420), _blob(H, W, 900, 1890, 150, 210)]
    want, want_stats = im, []
    for m in masks:
        want_stats.append(fgm.lighting_stats_host(want, m))
        want = fgm.handle_lighting_host(want, m)
    runs = []
    for _ in range(2):
        t = _c(im)
        for m, ws in zip(masks, want_stats):
            stats = torch.empty(9, dtype=torch.int64, device="cuda")
            fgm.handle_lighting(t, _c(m), stats=stats)
            assert np.array_equal(stats.cpu().numpy(), ws)
        runs.append(t.cpu().numpy())
    assert np.array_equal(runs[0], want)
    assert np.array_equal(runs[1], runs[0])


def _oracle_frame(bg, depth, sem, instances, lighting=None):
    """generate_images.py:80-185 for one frame with the oracle's pieces (the helper of tests/test_foreground.py) and, with `lighting`,
    fuse()'s handle_lighting after each paste (utils_render.py:300) through the host model"""
    bg, depth, sem = bg.copy(), depth.copy(), sem.copy()
    tm = tb = tocc = None
    occ = []
    for inst in instances:
        cat = inst["category"]
        r = of.bound_radius(inst["mask"], cat)
        bg, depth, sem, tested, o = of.occlusion_paste(bg, inst["image"], inst["mask"], depth, sem, inst["fg_depth"], cat)
        if lighting is not None:
            bg = fgm.handle_lighting_host(bg, tested, keep_background=lighting == "masked")
        occ.append(o)
        bound = of.get_bound_im(inst["mask"], r)
        mask = of.set_diff(inst["mask"], bound)
        tb = bound if tb is None else of.fuse_bound(tm, tb, bound, mask)
        tm = mask if tm is None else of.mask_union(tm, mask)
        if cat == "vehicle":
            tocc = tested if tocc is None else of.mask_union(tocc, tested)
    return dict(fuse=of.fuse_bound_and_im(bg, tb), mask=tm, bound=tb, occluded_mask=tocc, depth=depth, semantic=sem, occlusion=occ)


@gpu
def test_composite_frame_with_lighting_vs_oracle():
    """96 x 128: a vehicle, a person, an empty instance and a second vehicle overlapping the first, with lighting="frame" (the
    reference) and "masked"; lighting=None is the call without the keyword"""
    rng = np.random.default_rng(4)
    H, W = 96, 128
    bg = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = (rng.integers(256, 80 * 256, (H, W)) / 256.).astype(np.float32)
    sem = rng.integers(0, 19, (H, W)).astype(np.uint8)
    inst = []
    for cy, cx, ry, rx, cat in ((50, 40, 20, 30, "vehicle"), (55, 70, 30, 9, "person"), (0, 0, 0, 0, "vehicle"), (46, 56, 16, 28, "vehicle")):
        m = _blob(H, W, cy, cx, max(ry, 1), max(rx, 1)) * np.uint8(ry > 0)
        inst.append(dict(image=rng.integers(0, 256, (H, W, 3)).astype(np.uint8), mask=m.astype(np.uint8),
                         fg_depth=(rng.random((H, W)) * 70 + 1).astype(np.float32), category=cat))
    dev = lambda: [dict(image=_c(i["image"]), mask=_c(i["mask"]), fg_depth=_c(i["fg_depth"]), category=i["category"]) for i in inst]
    outs = {}
    for mode in ("frame", "masked", None):
        ref = _oracle_frame(bg, depth.astype(np.float64), sem, inst, mode)
        out = outs[mode] = fgm.composite_frame(_c(bg), _c(depth), _c(sem), dev(), lighting=mode)
        for k in ("fuse", "mask", "bound", "occluded_mask", "semantic"):
            assert np.array_equal(out[k].cpu().numpy(), ref[k]), (mode, k)
        assert np.array_equal(out["depth"].cpu().numpy().astype(np.float64), ref["depth"]), mode
        assert [float(o) for o in out["occlusion"]] == [float(o) for o in ref["occlusion"]]
    plain = fgm.composite_frame(_c(bg), _c(depth), _c(sem), dev())
    assert sorted(plain) == sorted(outs[None]) == sorted(outs["frame"])
    for k in ("fuse", "mask", "bound", "occluded_mask", "semantic", "depth"):
        assert torch.equal(plain[k], outs[None][k]), k
    assert not torch.equal(outs["frame"]["fuse"], plain["fuse"]) and not torch.equal(outs["masked"]["fuse"], outs["frame"]["fuse"])


@gpu
def test_handle_lighting_replays_from_a_graph():
    """handle_lighting with a preallocated stats tensor captured in one graph (a single-stream chain) and replayed on a second frame's
    content copied into the captured tensors"""
    cases = _cases()
    (im1, mask1), (im2, mask2) = cases["interior"], cases["dark_on_bright"]
    im, mask, stats = _c(im1), _c(mask1), torch.empty(9, dtype=torch.int64, device="cuda")
    fgm.handle_lighting(im.clone(), mask, stats=stats)                                       # (loads the kernels outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fgm.handle_lighting(im, mask, stats=stats)
    for src_im, src_mask in ((im2, mask2), (im1, mask1)):
        im.copy_(_c(src_im)); mask.copy_(_c(src_mask)); stats.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_stats = _c(src_im), torch.empty(9, dtype=torch.int64, device="cuda")
        fgm.handle_lighting(eager, _c(src_mask), stats=eager_stats)
        assert torch.equal(im, eager) and torch.equal(stats, eager_stats)
        assert np.array_equal(im.cpu().numpy(), fgm.handle_lighting_host(src_im, src_mask))
