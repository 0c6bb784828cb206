"""The DCN bilinear sampling rule (monoflex_amd/csrc/dcn_sample_math.h: the one statement every DCN kernel calls) without a GPU: the header
compiled for the host (tests/shim/dcn_sample_host.cpp, -ffp-contract=off) against

  * a numpy restatement below (float32 where the header is float32, so EXACT equality: position, inside, floor fractions lh / lw / hh / hw,
    clamped integer corner, validity and clamped index of each corner; the four corner weights and the eight coordinate-derivative
    coefficients too -- the float64 product of two float32 values is exact, so its float32 rounding IS the float32 product: no quantity
    needs the 1-ulp allowance), and
  * oracle/dcn_v2_ref.c: its im2col of an image of H * W impulse channels is, per (output pixel, tap), the map of `valid ? weight : 0` over the
    input pixels -- inside, validity, integer corners and weights in one exact comparison.  The oracle needs a real convolution, so it
    runs on the geometries that have at least one output pixel (a 1-wide map under pad 0 has none; the numpy form covers those).

Maps 1x1, 1x7, 5x1, 12x20; 3x3 taps with stride 1 / pad 1, and the general form with stride 2 / 1, pad 0 / 2, dilation 1 / 2 per axis and its
transpose.  The inputs populate every case of the rule; the census is asserted."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAPS = [(1, 1), (1, 7), (5, 1), (12, 20)]
# (form of the shim: 0 = the 3x3 functions, else the general ones; (stride_h, stride_w), (pad_h, pad_w), (dil_h, dil_w))
GEOMS = [(0, (1, 1), (1, 1), (1, 1)), (1, (2, 1), (0, 2), (1, 2)), (2, (1, 2), (2, 0), (2, 1))]
WILD = np.array([1e9, -1e9, 3e38, -3e38, np.inf, -np.inf, np.nan], dtype=np.float32)
LO, HI, HI_WIDE = -24, 30000, 1 << 30
f32 = np.float32


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "libdcn_sample_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "dcn_sample_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_dcn_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 8
    lib.shim_dcn_sample.restype = None
    lib.shim_dcn_sample_consts.argtypes = [ctypes.c_void_p]
    return lib


def out_size(n, s, p, d):
    return (n + 2 * p - (d * 2 + 1)) // s + 1


def make_case(H, W, geom, seed):
    """Samples on the (output pixel, tap) grid, repeated; every sample drawn from one of the categories of the rule."""
    form, (sh, sw), (ph, pw), (dh_, dw_) = geom
    Ho, Wo = out_size(H, sh, ph, dh_), out_size(W, sw, pw, dw_)
    has_conv = Ho >= 1 and Wo >= 1
    gh, gw = max(Ho, 1), max(Wo, 1)
    reps = max(2, 1800 // (gh * gw * 9) + 1)
    rng = np.random.default_rng(seed)
    oh, ow, tap = [a.reshape(-1) for a in np.meshgrid(np.arange(gh), np.arange(gw), np.arange(9), indexing="ij")]
    oh, ow, tap = [np.tile(a, reps).astype(np.int32) for a in (oh, ow, tap)]
    n = oh.size
    base = np.stack([oh * sh - ph + (tap // 3) * dh_, ow * sw - pw + (tap % 3) * dw_], 1).astype(np.float64)
    size = np.array([H, W], dtype=np.float64)
    cat = rng.choice(9, n, p=[0.22, 0.08, 0.08, 0.07, 0.07, 0.07, 0.07, 0.14, 0.20])
    tgt = rng.random((n, 2)) * size - rng.random((n, 2)) * (rng.random((n, 2)) < 0.15)       # 0: anywhere inside (-1, H) x (-1, W), mostly [0, H)
    k = cat == 1                                                                             # 1: integer coordinates inside the map
    tgt[k] = np.floor(rng.random((k.sum(), 2)) * size)
    k = cat == 2                                                                             # 2: exactly -1 or H on one axis (the other inside)
    ax, side = rng.integers(0, 2, n), rng.integers(0, 2, n)
    edge = np.where(side == 0, -1.0, size[ax])
    tgt[k, ax[k]] = edge[k]
    for c, (axis, hi) in zip((3, 4, 5, 6), ((0, 0), (0, 1), (1, 0), (1, 1))):                # 3..6: the border bands (-1, 0), (H-1, H) of either axis
        k = cat == c
        frac = 0.02 + 0.96 * rng.random(k.sum())
        tgt[k, axis] = (size[axis] - 1 + frac) if hi else (-1 + frac)
    k = cat == 7                                                                             # 7: misses the map by up to ~2 H on one or both axes
    miss = (1.0 + rng.random((n, 2)) * 2 * size) * np.where(rng.random((n, 2)) < 0.5, -1, 1)
    both = rng.random((n, 2)) < 0.6
    both[np.arange(n), ax] = True
    tgt[k] = np.where(both, np.where(miss < 0, -1 + miss, size + miss), tgt)[k]
    d = (tgt - base).astype(f32)
    k = cat == 8                                                                             # 8: wild values on one or both axes
    wild = WILD[rng.integers(0, WILD.size, (n, 2))]
    d[k] = np.where(both, wild, d)[k]
    return dict(H=H, W=W, form=form, geom=np.array([H, W, 3, sh, sw, ph, pw, dh_, dw_], dtype=np.int32), Ho=Ho, Wo=Wo, has_conv=has_conv, reps=reps,
                oh=oh, ow=ow, tap=tap, dh=np.ascontiguousarray(d[:, 0]), dw=np.ascontiguousarray(d[:, 1]), base=base, cat=cat, n=n)


def run_shim(lib, c):
    fl, ints, cw = np.zeros((c["n"], 10), f32), np.zeros((c["n"], 18), np.int32), np.zeros((c["n"], 8), f32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                          # noqa: E731
    lib.shim_dcn_sample(p(c["geom"]), c["form"], c["n"], p(c["oh"]), p(c["ow"]), p(c["tap"]), p(c["dh"]), p(c["dw"]), p(fl), p(ints), p(cw))
    return fl, ints, cw


def restate(c):
    """The rule in numpy.  float32 wherever the header is, float64 for the products (exact for float32 factors)."""
    H, W = c["H"], c["W"]
    hi_clamp = HI if c["form"] == 0 else HI_WIDE
    with np.errstate(invalid="ignore", over="ignore"):
        h, w = c["base"][:, 0].astype(f32) + c["dh"], c["base"][:, 1].astype(f32) + c["dw"]
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hf, wf = np.floor(h), np.floor(w)
        lh, lw = h - hf, w - wf
        hh, hw = f32(1) - lh, f32(1) - lw
        h0 = np.fmin(np.fmax(hf, f32(LO)), f32(hi_clamp)).astype(np.int64)                  # fmax(NaN, LO) = LO, as fmaxf
        w0 = np.fmin(np.fmax(wf, f32(LO)), f32(hi_clamp)).astype(np.int64)
        hc, wc = np.stack([h0, h0, h0 + 1, h0 + 1], 1), np.stack([w0, w0 + 1, w0, w0 + 1], 1)
        valid = inside[:, None] & (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
        a, b = np.stack([hh, hh, lh, lh], 1).astype(np.float64), np.stack([hw, lw, hw, lw], 1).astype(np.float64)
        weight = (a * b).astype(f32)
        coord = np.stack([-hw, -lw, hw, lw, -hh, hh, -lh, lh], 1)
    return dict(h=h, w=w, inside=inside, lh=lh, lw=lw, hh=hh, hw=hw, h0=h0, w0=w0, valid=valid, ch=np.clip(hc, 0, H - 1), cw=np.clip(wc, 0, W - 1),
                weight=weight, coord=coord)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


CASES = [(hw, g) for hw in MAPS for g in GEOMS]


def test_row_layout_and_clamp_constants(shim):
    out = np.zeros(8, np.int32)
    shim.shim_dcn_sample_consts(out.ctypes.data_as(ctypes.c_void_p))
    assert out.tolist() == [32, 18, 10, 11, 23, LO, HI, HI_WIDE]
    assert LO <= -2 and LO + 32 >= 0 and HI + 32 < (1 << 15)                                 # the (h0 + 32) | ((w0 + 32) << 16) packing of dcn_lds / dcn_patch


@pytest.mark.parametrize("hw,geom", CASES)
def test_header_vs_numpy_restatement(shim, hw, geom):
    c = make_case(hw[0], hw[1], geom, seed=1000 * hw[0] + 10 * hw[1] + geom[0])
    fl, ints, cwt = run_shim(shim, c)
    r = restate(c)
    H, W, n = c["H"], c["W"], c["n"]
    # ---- census: every case of the rule is populated (by what the header itself was given: the float32 positions)
    h, w, ins = r["h"], r["w"], r["inside"]
    fin = np.isfinite(h) & np.isfinite(w)
    with np.errstate(invalid="ignore"):
        wild = ~fin | (np.abs(h) >= 1e8) | (np.abs(w) >= 1e8)
        band = lambda v, lo: ins & (v > lo) & (v < lo + 1)                                   # noqa: E731
        census = {
            "strictly inside": ins.sum(), "wild": wild.sum(),
            "band h (-1, 0)": band(h, -1).sum(), "band h (H-1, H)": band(h, H - 1).sum(),
            "band w (-1, 0)": band(w, -1).sum(), "band w (W-1, W)": band(w, W - 1).sum(),
            "miss": (~ins & ~wild & ((h < -1) | (h > H) | (w < -1) | (w > W))).sum(),
        }
        few = {"integer": (ins & (r["lh"] == 0) & (r["lw"] == 0)).sum(),
               "h == -1": (h == -1).sum(), "h == H": (h == H).sum(), "w == -1": (w == -1).sum(), "w == W": (w == W).sum()}
    for k, v in census.items():
        assert v >= 0.05 * n, (k, int(v), n)
    for k, v in few.items():
        assert v >= 4, (k, int(v), n)
    assert not ins[(h == -1) | (h == H) | (w == -1) | (w == W)].any()                        # strict on both sides
    for v in WILD:
        assert (np.isnan(c["dh"]).any() and np.isnan(c["dw"]).any()) if np.isnan(v) else ((c["dh"] == v).any() and (c["dw"] == v).any()), v
    # ---- exact agreement
    assert same(ints[:, 0], c["tap"] // 3) and same(ints[:, 1], c["tap"] % 3)
    assert same(fl[:, 0], h) and same(fl[:, 1], w)
    assert same(ints[:, 2] != 0, ins)
    for j, name in enumerate(("lh", "lw", "hh", "hw")):
        assert same(fl[:, 2 + j], r[name]), name
    assert same(ints[:, 3], r["h0"]) and same(ints[:, 4], r["w0"])
    assert same(ints[:, 5:9] != 0, r["valid"])
    assert same(ints[:, 9:17:2], r["ch"]) and same(ints[:, 10:17:2], r["cw"])
    assert same(fl[:, 6:10], r["weight"]) and same(cwt, r["coord"])
    assert ints[:, 17].all()                                                                 # sample_inside == sample, in_map == corner_valid where inside
    # ---- what the rule promises for wild and missing samples
    out = ~ins
    assert wild.sum() and not ins[wild].any() and not (ints[out, 5:9] != 0).any()
    hi_clamp = HI if c["form"] == 0 else HI_WIDE
    assert ints[:, 3:5].min() >= LO and ints[:, 3:5].max() <= hi_clamp
    assert ints[:, 9:17:2].min() >= 0 and ints[:, 9:17:2].max() <= H - 1 and ints[:, 10:17:2].min() >= 0 and ints[:, 10:17:2].max() <= W - 1
    assert (ints[ins, 3] >= -1).all() and (ints[ins, 3] <= H - 1).all() and (ints[ins, 4] >= -1).all() and (ints[ins, 4] <= W - 1).all()


@pytest.mark.parametrize("hw,geom", [(hw, g) for hw, g in CASES if out_size(hw[0], g[1][0], g[2][0], g[3][0]) >= 1 and out_size(hw[1], g[1][1], g[2][1], g[3][1]) >= 1])
def test_header_vs_c_oracle(shim, hw, geom):
    from oracle import dcn_ref
    c = make_case(hw[0], hw[1], geom, seed=1000 * hw[0] + 10 * hw[1] + geom[0])
    fl, ints, _ = run_shim(shim, c)
    H, W, Ho, Wo = c["H"], c["W"], c["Ho"], c["Wo"]
    (sh, sw), (ph, pw), (dh_, dw_) = geom[1:]
    P, C = Ho * Wo, H * W
    im = np.eye(C, dtype=f32).reshape(C, H, W)                                               # channel c = the impulse at input pixel c
    mask = np.ones((9, Ho, Wo), f32)
    per = P * 9
    L_ = dcn_ref.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                          # noqa: E731
    for rep in range(c["reps"]):
        sl = slice(rep * per, (rep + 1) * per)
        off = np.zeros((18, Ho, Wo), f32)
        off[0::2] = c["dh"][sl].reshape(Ho, Wo, 9).transpose(2, 0, 1)
        off[1::2] = c["dw"][sl].reshape(Ho, Wo, 9).transpose(2, 0, 1)
        off = np.ascontiguousarray(off)
        cols = np.full((C, 9, P), -7.0, f32)
        assert L_.dcn_ref_im2col_image(p(im), p(off), p(mask), p(cols), C, H, W, 3, 3, sh, sw, ph, pw, dh_, dw_, 1) == 0
        want = np.zeros((C, 9, P), f32)
        pix = (c["oh"][sl] * Wo + c["ow"][sl]).astype(np.int64)
        for q in range(4):
            v = ints[sl, 5 + q] != 0
            want[(ints[sl, 9 + 2 * q] * W + ints[sl, 10 + 2 * q])[v], c["tap"][sl][v], pix[v]] = fl[sl, 6 + q][v]
        assert np.array_equal(cols, want), (rep, int((cols != want).sum()))
