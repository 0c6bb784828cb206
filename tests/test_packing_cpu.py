"""The weight layouts of monoflex_amd/packing.py, each against its index formula written out as plain loops (CPU, no GPU needed).

The formulas are the ones the kernels' fragment loads are written to (the comments in packing.py); nothing below calls the function
under test to make its own expectation."""
import itertools

import numpy as np
import pytest
import torch

from monoflex_amd import ops, packing as P

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "f16x2": P.F16X2}


def _np(t):
    return t.detach().float().numpy()


def _halves(t):
    """float32-typed split-precision tensor -> its fp16 halves as float32 numpy, last axis twice as long."""
    return t.contiguous().view(torch.float16).float().numpy()


def _hi_lo(x):
    """The split-precision rule restated: (fp16(x), fp16(x - fp16(x))) of a float32 numpy array, as float32."""
    hi = x.astype(np.float16)
    return hi.astype(np.float32), (x - hi.astype(np.float32)).astype(np.float16).astype(np.float32)


def test_packing_is_not_a_second_home_of_ops():
    assert P.__name__ == "monoflex_amd.packing" and "ops" not in vars(P)
    for name in ("pack_conv", "pack_stem", "pack_cat", "pack_heads", "PackedConv", "PackedCat", "PackedHeads", "F16X2", "fold_bn", "cout_pad",
                 "fragment_major", "split_chunks", "pair_steps", "add_f16_fragments", "dcn_ps_pack", "pack_upsample", "split_weight_scale"):
        assert getattr(ops, name) is getattr(P, name), name


@pytest.mark.parametrize("E,tag", [(4, torch.float32), (8, torch.bfloat16)])
def test_fragment_major_index_formula(E, tag):
    K = 128 // (16 // E)                                            # a 128-byte K row
    w = torch.arange(32 * K).view(32, K)                            # distinct integers
    f = P.fragment_major(w, tag)
    assert tuple(f.shape) == (2, K // (4 * E), 4, 16, E)
    for nf, ks, kq, n, e in itertools.product(range(2), range(K // (4 * E)), range(4), range(16), range(E)):
        assert int(f[nf, ks, kq, n, e]) == int(w[16 * nf + n, (4 * ks + kq) * E + e])


def test_split_chunks_layout_and_error_bound():
    """Every 16-byte chunk is [4 hi | 4 lo] of its four values, and hi + lo reproduces x to 2^-22 |x|: hi = fp16(x) is off by at most
    2^-11 |x|, lo = fp16(x - hi) by at most 2^-11 of THAT -- where x - hi is a normal fp16 number.  A residual below 2^-14 is an fp16
    subnormal (spacing 2^-24, error up to 2^-25), so the relative bound follows for |x| >= 2^-3 only (2^-25 = 2^-22 * 2^-3); over the rest
    of fp16's normal range what holds is max(2^-22 |x|, 2^-25), which is why pack_* scale the weights up (split_weight_scale)."""
    g = torch.Generator().manual_seed(0)
    mag = torch.cat((2.0 ** (torch.rand(6, 16, generator=g) * 13 - 3), 2.0 ** (torch.rand(6, 16, generator=g) * 11 - 14)))    # [2^-3, 2^10), [2^-14, 2^-3)
    x = mag * (1 - 2 * (torch.rand(12, 16, generator=g) < 0.5).float())
    out = P.split_chunks(x)
    assert out.dtype == torch.float32 and out.shape == x.shape
    h = _halves(out).reshape(12, 4, 8)                              # [row][chunk][4 hi | 4 lo]
    xs = x.numpy().reshape(12, 4, 4)
    for r, c, i in itertools.product(range(12), range(4), range(4)):
        v = float(xs[r, c, i])
        hi, lo = float(h[r, c, i]), float(h[r, c, 4 + i])
        assert hi == float(np.float16(v))
        assert lo == float(np.float16(np.float32(v) - np.float32(hi)))
        err = abs(float(np.float32(hi) + np.float32(lo)) - v)
        assert err <= max(2.0 ** -22 * abs(v), 2.0 ** -25)
        if abs(v) >= 2.0 ** -3:
            assert err <= 2.0 ** -22 * abs(v)
    hi, lo = P.split_halves(x)
    assert hi.dtype == lo.dtype == torch.float16 and hi.shape == lo.shape == x.shape
    assert torch.equal(hi, x.to(torch.float16)) and torch.equal(lo, (x - x.to(torch.float16).float()).to(torch.float16))


def test_pair_steps_index_map():
    x = torch.arange(2 * 4 * 3 * 4, dtype=torch.float32).view(2, 4, 3, 4)        # [a][step][m][hi hi | lo lo]
    y = P.pair_steps(x, 1)
    assert tuple(y.shape) == (2, 2, 2, 3, 4)                        # [a][pair][hi | lo][m][dwords of step 2p | of step 2p + 1]
    for a, p, h, m, s, j in itertools.product(range(2), range(2), range(2), range(3), range(2), range(2)):
        assert float(y[a, p, h, m, 2 * s + j]) == float(x[a, 2 * p + s, m, 2 * h + j])


def _is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def _distinct_fp16(*shape):
    """Distinct, finite, exactly-fp16 values (consecutive bit patterns of normal numbers) as float32."""
    n = int(np.prod(shape))
    assert n < 30000
    return (torch.arange(n, dtype=torch.int16) + 1024).view(torch.float16).float().view(*shape)


def _pair_fragments_by_formula(w, cout_pad):
    """dcn_pair_fragments by its docstring: lane (kq, n) of k-step j of slice s holds tap 2j + (kq >> 1), channels 16 s + 8 (kq & 1) .. + 7."""
    Cout, Cin = w.shape[:2]
    out = np.zeros((cout_pad // 16, Cin // 16 * 5, 4, 16, 8), np.float32)
    for nf, s, j, kq, n in itertools.product(range(cout_pad // 16), range(Cin // 16), range(5), range(4), range(16)):
        tap, row = 2 * j + (kq >> 1), 16 * nf + n
        if tap < 9 and row < Cout:                                  # the tenth tap and the padding rows are zero
            c0 = 16 * s + 8 * (kq & 1)
            out[nf, 5 * s + j, kq, n] = w[row, c0:c0 + 8, tap // 3, tap % 3]
    return out


def test_dcn_pair_fragments_index_formula():
    w = _distinct_fp16(64, 32, 3, 3)
    f = P.dcn_pair_fragments(w, 64)
    assert f.dtype == torch.float16 and tuple(f.shape) == (4, 10, 4, 16, 8)
    assert np.array_equal(_np(f), _pair_fragments_by_formula(w.numpy(), 64))
    assert float(f[:, 4::5, 2:].abs().max()) == 0.0                 # k-step 4, kq >= 2: the tenth tap


def test_pack_conv_geometry_and_split_scale():
    g = torch.Generator().manual_seed(1)
    for cin, kpad in ((8, 32), (32, 32), (64, 64), (128, 128)):     # bf16 1x1: a K of up to 64 bytes is ONE 64-byte row (32 elements), longer ones pad to 128 bytes
        p = P.pack_conv(torch.randn(20, cin, 1, 1, generator=g), torch.bfloat16)
        assert p.K_pad == kpad and p.w.shape == (32, kpad) and p.w_frag is None and p.split_scale == 1.0 and not p.split
    assert P.pack_conv(torch.randn(16, 8, 1, 1, generator=g), torch.float32).K_pad == 16          # fp32: 64 bytes are 16 elements
    scale = torch.rand(64, generator=g) + 0.5
    for cin in (16, 32, 64):
        w = torch.randn(64, cin, 3, 3, generator=g) * 0.05
        p = P.pack_conv(w, P.F16X2, scale, None, stride=1, pad=1)
        m = float(w.abs().max()) * p.split_scale
        assert p.split and 2.0 ** 11 <= m < 2.0 ** 12 and p.split_scale == 2.0 ** round(np.log2(p.split_scale))
        assert torch.equal(p.scale * p.split_scale, scale)          # a power of two: exact
        assert p.w_frag is not None and (p.w_frag_pair is not None) == (cin >= 32)
        q = P.pack_conv(w, torch.bfloat16, scale, None, stride=1, pad=1)
        assert q.w_frag is not None and q.w_frag_pair is None and q.split_scale == 1.0 and torch.equal(q.scale, scale)
    ws = torch.randn(16, 3, 7, 7, generator=g) * 0.1
    for cout in (16, 32):                                           # the dedicated 16-channel kernel's pack and the generic one
        s = torch.rand(cout, generator=g) + 0.5
        ps = P.pack_stem(torch.randn(cout, 3, 7, 7, generator=g) * 0.1, P.F16X2, s, torch.zeros(cout))
        assert ps.split and ps.split_scale > 1.0 and torch.equal(ps.scale * ps.split_scale, s)
    assert P.pack_stem(ws, torch.bfloat16, torch.ones(16), torch.zeros(16)).split_scale == 1.0
    p = P.pack_conv(torch.randn(8, 16, 1, 1), torch.float32)
    assert (p.transient, p.entry, p.f1_w160, p.ps) == (False, None, None, None)
    with pytest.raises(TypeError):
        P.PackedConv(p.w, None, None, 1, 1, 1, 0, 0, 1, 16, 8, 16, 16, 0, transcient=True)     # a misspelt field is an error, not "absent"


def _unfragment(flat, rows, K, E=8):
    """Inverse of fragment_major by its formula: flat [rows/16][K/(4E)][4 kq][16 n][E] -> [rows][K]."""
    f = flat.reshape(rows // 16, K // (4 * E), 4, 16, E)
    out = np.zeros((rows, K), np.float32)
    for nf, ks, kq, n in itertools.product(range(rows // 16), range(K // (4 * E)), range(4), range(16)):
        out[16 * nf + n, (4 * ks + kq) * E:(4 * ks + kq + 1) * E] = f[nf, ks, kq, n]
    return out


def test_add_f16_fragments_split_halves_decode_to_the_scaled_weights():
    g = torch.Generator().manual_seed(2)
    Cout, Cin = 48, 32                                              # rows padded to 64
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 0.75 + 0.25) * 0.03 * (1 - 2 * (torch.rand(Cout, Cin, 3, 3, generator=g) < 0.5).float())
    p = P.add_f16_fragments(P.pack_conv(w, P.F16X2, None, torch.zeros(Cout), stride=1, pad=1), w)
    K = 9 * Cin
    assert p.K_pad == K and p.Cout_pad == 64 and p.w_frag_f16.dtype == torch.float16 and p.w_frag_f16.numel() == 2 * 64 * K
    sw = np.zeros((64, K), np.float32)                              # split_scale * w as [n][(tap, c)], padding rows zero
    sw[:Cout] = (w * p.split_scale).permute(0, 2, 3, 1).reshape(Cout, K).numpy()
    hi, lo = _hi_lo(sw)
    fr = _np(p.w_frag_f16).reshape(2, -1)
    assert np.array_equal(_unfragment(fr[0], 64, K), hi) and np.array_equal(_unfragment(fr[1], 64, K), lo)       # fragment_major of hi, then of lo
    assert np.abs(hi.astype(np.float64) + lo - sw).max() <= 2.0 ** -22 * np.abs(sw).max() and np.abs(sw[:Cout]).min() >= 2.0 ** -3
    pr = _np(p.w_pair_f16).reshape(2, 4, Cin // 16 * 5, 4, 16, 8)
    w4 = (w * p.split_scale).numpy()
    h4, l4 = _hi_lo(w4)
    assert np.array_equal(pr[0], _pair_fragments_by_formula(h4, 64)) and np.array_equal(pr[1], _pair_fragments_by_formula(l4, 64))
    # 16-bit modes: the plain fp16 weights in both orders
    q = P.add_f16_fragments(P.pack_conv(w, torch.bfloat16, None, torch.zeros(Cout), stride=1, pad=1), w)
    assert q.K_pad == 320                                           # bf16: 288 elements pad to whole 128-byte rows
    w16 = np.zeros((64, q.K_pad), np.float32)
    w16[:Cout, :K] = w.permute(0, 2, 3, 1).reshape(Cout, K).numpy().astype(np.float16)
    assert np.array_equal(_unfragment(_np(q.w_frag_f16).reshape(-1), 64, q.K_pad), w16)
    assert np.array_equal(_np(q.w_pair_f16), _pair_fragments_by_formula(w.numpy().astype(np.float16).astype(np.float32), 64))


# the operand shapes of the network as tests/test_gpu_train.py::test_batched_operand_packing_equals_the_single_operand_kernel lists them: (Cout, Cin, k, mode)
NETWORK_OPERANDS = [(64, 64, 3, 0), (64, 64, 3, 1), (27, 64, 3, 0), (64, 27, 3, 1), (256, 64, 3, 0), (256, 64, 3, 1), (512, 512, 3, 0), (512, 512, 3, 1),
                    (128, 64, 3, 0), (128, 64, 3, 1), (64, 128, 1, 0), (64, 128, 1, 1), (3, 256, 1, 0), (3, 256, 1, 1), (20, 256, 1, 0), (32, 16, 3, 0),
                    (32, 16, 3, 1), (1024, 1024, 3, 0), (16, 16, 1, 0)]


@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_operand_geometry_is_what_the_training_registry_allocates(dt):
    from monoflex_amd import autograd as AG
    dtype, E = DT[dt], 4 if dt == "fp32" else 8
    reg = AG._PackRegistry()
    for cout, cin, k, mode in NETWORK_OPERANDS:
        w = torch.empty(cout, cin, k, k)
        rows_src, ck_src = (cout, cin) if mode == 0 else (cin, cout)
        ck = max(E, (ck_src + E - 1) // E * E)
        if k > 1:
            ck = 1 << (ck - 1).bit_length()
        for rows, stride in itertools.product({(rows_src + 15) // 16 * 16, P._pad_channels(rows_src, dtype)}, (1, 2) if k == 3 else (1,)):
            K_pad, cp, frag = P.operand_geometry(k, k, ck, rows, stride, k // 2, k // 2, E)
            e = reg.lookup(w, dtype, mode, rows, ck, stride, k // 2, k // 2, register=False)
            assert tuple(e["packed"].shape) == (cp, K_pad) and (e["cp"], e["K_pad"]) == (cp, K_pad) and e["packed"].dtype == dtype
            assert (e["frag"] is not None) == frag == (k == 3) and (not frag or e["frag"].shape == e["packed"].shape)
            # the rule itself: whole 16-byte chunks, one 64-byte row or whole 128-byte rows, rows padded as the kernels' tiles need
            assert K_pad >= k * k * ck and K_pad % (4 * E) == 0 and (K_pad == 4 * E or K_pad % (8 * E) == 0) and K_pad - k * k * ck < 8 * E
            assert cp >= rows and (cp in (16, 32) or cp % 64 == 0)
    # written-out cases, through both callers: (k, channels per tap, rows, stride) -> (K_pad in BYTES, padded rows, fragment-major copy).  A K of
    # exactly 64 bytes (and anything shorter) is one 64-byte row, 65 .. 128 bytes one 128-byte row, 3x3 x 64 channels whole 128-byte rows
    for (k, ck_bytes, rows, stride), (kb, cp, frag) in {(1, 64, 64, 1): (64, 64, False), (1, 32, 20, 1): (64, 32, False), (1, 128, 16, 1): (128, 16, False),
                                                        (1, 96, 64, 1): (128, 64, False), (3, 256, 27, 1): (2304, 32, True), (3, 256, 64, 2): (2304, 64, True),
                                                        (3, 64, 130, 1): (640, 192, True)}.items():
        ck, esz = ck_bytes * E // 16, 16 // E
        assert P.operand_geometry(k, k, ck, rows, stride, k // 2, k // 2, E) == (kb // esz, cp, frag)
        e = reg.lookup(torch.empty(rows, ck, k, k), dtype, 0, rows, ck, stride, k // 2, k // 2, register=False)
        assert tuple(e["packed"].shape) == (cp, kb // esz) and (e["frag"] is not None) == frag
        if _is_pow2(ck):
            p = P.pack_conv(torch.zeros(rows, ck, k, k), dtype, stride=stride, pad=k // 2)
            assert (p.K_pad, p.Cout_pad, p.w_frag is not None) == (kb // esz, cp, frag)
    assert not reg.entries                                          # register=False remembers nothing
    with pytest.raises(ValueError, match="channels per tap must be a power of two"):
        reg.lookup(torch.empty(64, 24, 3, 3), dtype, 0, 64, 24, 1, 1, 1, register=False)
    reg.lookup(torch.empty(64, 24, 1, 1), dtype, 0, 64, 24, 1, 0, 0, register=False)            # ... any multiple of a chunk for 1x1
    with pytest.raises(ValueError, match="pack_conv: Cin must be a power of two"):
        P.pack_conv(torch.empty(64, 24, 1, 1), dtype)


def test_pad_channels_and_cout_pad():
    assert [P.cout_pad(c) for c in (1, 16, 17, 32, 33, 64, 65, 576)] == [16, 16, 32, 32, 64, 64, 128, 576]
    assert [P._pad_channels(n, torch.float32) for n in (1, 3, 4, 5, 27, 50, 64, 65)] == [4, 4, 4, 8, 32, 64, 64, 128]
    assert [P._pad_channels(n, torch.bfloat16) for n in (1, 3, 8, 9, 27, 64, 200)] == [8, 8, 8, 16, 32, 64, 256]


@pytest.fixture(scope="module")
def heads_input():
    g = torch.Generator().manual_seed(3)
    w3 = [torch.randn(256, 64, 3, 3, generator=g) * 0.05 for _ in range(2)]
    folds = [(torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)) for _ in range(2)]
    w1x1 = [torch.randn(3, 256, 1, 1, generator=g) * 0.1, torch.randn(5, 256, 1, 1, generator=g) * 0.1]
    b1x1 = [torch.randn(3, generator=g), torch.randn(5, generator=g)]
    return w3, folds, w1x1, b1x1


@pytest.mark.parametrize("dt", ["fp32", "bf16", "f16x2"])
def test_pack_heads_channel_formulas(heads_input, dt):
    w3, folds, w1x1, b1x1 = heads_input
    tag = DT[dt]
    p = P.pack_heads(w3, folds, w1x1, b1x1, 3, [0, 8], 64, tag)
    assert (p.K_pad, p.ch_off, p.c_out, p.ld_out, p.split) == (576, [0, 8], [3, 5], 64, dt == "f16x2")
    w1 = np.stack([w.permute(0, 2, 3, 1).reshape(256, 576).numpy() for w in w3])                 # [b][trunk channel][k = tap * 64 + c]
    w2 = np.zeros((2, 32, 256), np.float32)
    b2 = np.zeros((2, 32), np.float32)
    for b in range(2):
        c = w1x1[b].shape[0]
        w2[b, :c], b2[b, :c] = w1x1[b].reshape(c, 256).numpy(), b1x1[b].numpy()
    assert np.array_equal(_np(p.bias2), b2)
    sc = np.concatenate([f[0].numpy() for f in folds])
    assert np.array_equal(_np(p.shift1), np.concatenate([f[1].numpy() for f in folds]))
    if dt == "f16x2":
        s1 = [P.split_weight_scale(torch.from_numpy(w1[b])) for b in range(2)]
        s2 = [P.split_weight_scale(torch.from_numpy(w2[b])) for b in range(2)]
        assert p.w2_scale == [1.0 / s for s in s2] and np.array_equal(_np(p.scale1), sc / np.repeat(np.float32(s1), 256))
        w1, w2 = w1 * np.float32(s1)[:, None, None], w2 * np.float32(s2)[:, None, None]
        W1, W2 = _halves(p.w1), _halves(p.w2)
        assert W1.shape == (2, 4, 18, 2, 4, 4, 16, 8) and W2.shape == (2, 4, 2, 2, 2, 4, 16, 8)
        h1, h2 = _hi_lo(w1), _hi_lo(w2)
        # 3x3: [branch][wn][step pair][hi | lo][j][kq][nl][4 of step 2p | 4 of step 2p + 1], channel 64 wn + 16 j + nl, k = (4 step + kq) * 4 + e
        for b, wn, sp, h, j, kq, nl, s in itertools.product(range(2), range(4), range(18), range(2), range(4), range(4), range(16), range(2)):
            k0 = (4 * (2 * sp + s) + kq) * 4
            assert np.array_equal(W1[b, wn, sp, h, j, kq, nl, 4 * s:4 * s + 4], h1[h][b, 64 * wn + 16 * j + nl, k0:k0 + 4])
        # 1x1: [branch][wn][kb pair][hi | lo][of][g][o_l][4 of kb 2p | 4 of kb 2p + 1], n = 64 wn + 16 kb + 4 g + e
        for b, wn, kp, h, of, gq, ol, s in itertools.product(range(2), range(4), range(2), range(2), range(2), range(4), range(16), range(2)):
            n0 = 64 * wn + 16 * (2 * kp + s) + 4 * gq
            assert np.array_equal(W2[b, wn, kp, h, of, gq, ol, 4 * s:4 * s + 4], h2[h][b, 16 * of + ol, n0:n0 + 4])
        assert p.w1_32 is None and p.w2_32 is None
        return
    assert p.w2_scale is None and np.array_equal(_np(p.scale1), sc)
    cast = lambda a: torch.from_numpy(a).to(tag).float().numpy()                                 # noqa: E731  (element-wise: commutes with the layout)
    w1, w2 = cast(w1), cast(w2)
    W1, W2 = _np(p.w1), _np(p.w2)
    E = 4 if dt == "fp32" else 8
    assert p.w1.dtype == p.w2.dtype == tag and W1.shape == (2, 4, 576 // (4 * E), 4, 4, 16, E)
    # 3x3: [branch][wn 4][step][frag j 4][kq 4][nl 16][E], channel 64 wn + 16 j + nl, k = (4 step + kq) E + e
    for b, wn, s, j, kq, nl in itertools.product(range(2), range(4), range(576 // (4 * E)), range(4), range(4), range(16)):
        assert np.array_equal(W1[b, wn, s, j, kq, nl], w1[b, 64 * wn + 16 * j + nl, (4 * s + kq) * E:(4 * s + kq + 1) * E])
    if dt == "fp32":
        assert W2.shape == (2, 4, 4, 2, 4, 16, 4) and p.w1_32 is None and p.w2_32 is None
        # 1x1 f32: [branch][wn][kb 4][of 2][g 4][o_l 16][e 4], n = 64 wn + 16 kb + 4 g + e
        for b, wn, kb, of, gq, ol in itertools.product(range(2), range(4), range(4), range(2), range(4), range(16)):
            n0 = 64 * wn + 16 * kb + 4 * gq
            assert np.array_equal(W2[b, wn, kb, of, gq, ol], w2[b, 16 * of + ol, n0:n0 + 4])
        return
    assert W2.shape == (2, 4, 2, 2, 4, 16, 2, 4)
    # 1x1 bf16: [branch][wn][kb 2][of 2][g 4][o_l 16][half 2][q 4], n = 64 wn + 32 kb + 16 half + 4 g + q
    for b, wn, kb, of, gq, ol, half in itertools.product(range(2), range(4), range(2), range(2), range(4), range(16), range(2)):
        n0 = 64 * wn + 32 * kb + 16 * half + 4 * gq
        assert np.array_equal(W2[b, wn, kb, of, gq, ol, half], w2[b, 16 * of + ol, n0:n0 + 4])
    # the 32x32x16 MFMA form.  3x3: [branch][wn 4][K-step 36][rb 2][h 2][row 32][8], channel 64 wn + 32 rb + row, k = 16 s + 8 h + e
    A1, A2 = _np(p.w1_32), _np(p.w2_32)
    assert A1.shape == (2, 4, 36, 2, 2, 32, 8) and A2.shape == (2, 4, 2, 2, 2, 32, 2, 4) and p.w1_32.dtype == p.w2_32.dtype == tag
    for b, wn, s, rb, h, row in itertools.product(range(2), range(4), range(36), range(2), range(2), range(32)):
        assert np.array_equal(A1[b, wn, s, rb, h, row], w1[b, 64 * wn + 32 * rb + row, 16 * s + 8 * h:16 * s + 8 * h + 8])
    # 1x1: [branch][wn 4][rb 2][t 2][h 2][o 32][a 2][q 4], n = 64 wn + 32 rb + 16 t + 8 a + 4 h + q
    for b, wn, rb, t, h, o, a in itertools.product(range(2), range(4), range(2), range(2), range(2), range(32), range(2)):
        n0 = 64 * wn + 32 * rb + 16 * t + 8 * a + 4 * h
        assert np.array_equal(A2[b, wn, rb, t, h, o, a], w2[b, o, n0:n0 + 4])
