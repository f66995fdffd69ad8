"""TEST INFRASTRUCTURE (like everything under oracle/): a numpy restatement of the Winograd forms the fp32 kernels use since round 4, so that the
algebra the HIP kernels rely on is checked on the CPU against the plain convolution they replace.

  * denoiser_persist.hip, WINO instances (cm-tts_amd/csrc/weight_pack.cpp: to_wino_fragments): the gated k = 3, dilation-1 conv of
    ResidualBlock.forward (reference model/blocks.py:672) as F(2,3) over frame pairs;
  * conv_xlq.hip: conv_xlq_kernel (round 5): the dilation-1 ResBlock convs of HiFi-GAN as F(4,3) tap groups over output quads
    (conv1d_f43_taps below; dilation 3 / 5 by residue classes: conv1d_f43_taps_dil; conv_xlq_pair.hip's k = 3 pair as the chain of two: pair_f43);
  * denoiser_persist.hip, WINO == 2 instances (round 5; weight_pack.cpp: to_wino43_fragments): the same conv as F(4,3) over frame quads
    (conv1d_f43 below: the kernel's transforms in the kernel's operation order);
  * resblock_pair.hip: conv_xlw_kernel (cm-tts_amd/csrc/resblock_pair.h: WinoTab<k>, weight_pack.cpp: to_wino_iter_fragments): the k = 3 / 7 / 11 dilated convs of
    hifigan ResBlock1 (reference hifigan/models.py:96-103) over output pairs one dilation apart — groups of three taps as F(2,3), a remainder of two taps
    as F(2,2), a single remaining tap directly.

The second half restates the host-side weight packers (cm-tts_amd/csrc/weight_pack.cpp) as numpy index expressions — pack_weights /
unpack_weights — so that tests/test_weight_pack_cpu.py can compare the C++ that feeds the kernels bit for bit, and the algebra above can run on
the weights the packers emit.

Nothing here is imported by the product path (cm-tts_amd/, bench.py's timed region)."""
import numpy as np

# (accumulator, a, b, sgn, weight kind, tau): M[acc] += W_kind(tau) * (X(a) + sgn * X(b)); X(m) = the input m dilated taps to the right of the
# pair's first output's leftmost tap;  y(t) = (M0 + M1) + M2,  y(t + dil) = (M1 - M2) - M3          (resblock_pair.h: WinoEntry)
def _f23(t):
    return [(0, t, t + 2, -1, 0, t), (1, t + 1, t + 2, +1, 1, t), (2, t + 2, t + 1, -1, 2, t), (3, t + 1, t + 3, -1, 3, t)]


def _f22(t):
    return [(0, t, t + 1, -1, 0, t), (1, t + 1, 0, 0, 5, t), (3, t + 1, t + 2, -1, 6, t)]


def _one(t):
    return [(0, t, 0, 0, 0, t), (3, t + 1, 0, 0, 4, t)]


WINO_TAB = {3: _f23(0), 7: _f23(0) + _f23(3) + _one(6), 9: _f23(0) + _f23(3) + _f23(6), 11: _f23(0) + _f23(3) + _f23(6) + _f22(9)}      # 9: the FFT blocks' FFN conv (conv_xres.hip, WQ == 2)


def wino_weight(g, kind, tau):
    """g: [..., k] taps (last axis) -> the transformed weight of one table entry (weight_pack.cpp: wino23_weight and to_wino_iter_fragments)."""
    t = lambda i: g[..., i]
    return {0: lambda: t(tau), 1: lambda: 0.5 * (t(tau) + t(tau + 1) + t(tau + 2)), 2: lambda: 0.5 * (t(tau) - t(tau + 1) + t(tau + 2)),
            3: lambda: t(tau + 2), 4: lambda: -t(tau), 5: lambda: t(tau) + t(tau + 1), 6: lambda: t(tau + 1)}[kind]()


def conv1d_direct(x, w, dil=1):
    """x [Cin][T], w [Cout][Cin][k] -> y [Cout][T]: torch.nn.functional.conv1d(padding=dil * (k - 1) // 2, dilation=dil) (cross-correlation)."""
    cout, cin, k = w.shape
    T = x.shape[1]
    pad = dil * (k - 1) // 2
    xp = np.pad(x, ((0, 0), (pad, pad)))
    y = np.zeros((cout, T), x.dtype)
    for tap in range(k):
        y += w[:, :, tap] @ xp[:, tap * dil: tap * dil + T]
    return y


def conv1d_winograd(x, w, dil=1, U=None):
    """The same conv through the kernels' table: outputs in pairs (t, t + dil).  U: the table entries' transformed weights [entries][Cout][Cin]
    (unpack_weights of a packed stream) instead of the ones formed here."""
    cout, cin, k = w.shape
    T = x.shape[1]
    pad = dil * (k - 1) // 2
    tab = WINO_TAB[k]
    # first outputs of the pairs: blocks of 2 dil columns, the first dil of each block
    Tp = -(-T // (2 * dil)) * (2 * dil)
    xp = np.pad(x, ((0, 0), (pad, pad + (Tp - T) + dil * (k + 1))))
    t_first = np.asarray([q * 2 * dil + r for q in range(Tp // (2 * dil)) for r in range(dil)])
    X = lambda m: xp[:, t_first + m * dil]                      # [Cin][pairs]
    M = [np.zeros((cout, t_first.size), x.dtype) for _ in range(4)]
    for e, (acc, a, b, sgn, kind, tau) in enumerate(tab):
        v = X(a) + sgn * X(b) if sgn else X(a)
        M[acc] = M[acc] + (wino_weight(w, kind, tau) if U is None else U[e]).astype(x.dtype) @ v
    y = np.zeros((cout, Tp + dil), x.dtype)
    y[:, t_first] = (M[0] + M[1]) + M[2]
    y[:, t_first + dil] = (M[1] - M[2]) - M[3]
    return y[:, :T]


def f43_weights(w):
    """w [Cout][Cin][3] -> the six transformed weights U_p [Cout][Cin] (points 0, +-1, +-2, inf; weight_pack.cpp: wino43_weight forms them in
    double, the packers round once)."""
    g0, g1, g2 = (w[..., i].astype(np.float64) for i in range(3))
    return [g0 / 4.0, -(g0 + g1 + g2) / 6.0, -(g0 - g1 + g2) / 6.0, g0 / 24.0 + g1 / 12.0 + g2 / 6.0, g0 / 24.0 - g1 / 12.0 + g2 / 6.0, g2]


def conv1d_f43(x, w, U=None):
    """The k = 3, dilation-1, padding-1 conv through F(4,3): outputs in quads 4q .. 4q + 3 from inputs d0 .. d5 = x(4q - 1 .. 4q + 4)
    (denoiser_persist.hip, WINO == 2: transform4 / out4, same expressions).  U: the six transformed weights [6][Cout][Cin] (unpack_weights of a
    packed stream) instead of f43_weights(w)."""
    cout, cin, k = w.shape
    assert k == 3
    T = x.shape[1]
    Tq = -(-T // 4) * 4
    xp = np.pad(x, ((0, 0), (1, Tq - T + 4)))
    q0 = np.arange(0, Tq, 4)
    d = [xp[:, q0 + i] for i in range(6)]                      # [Cin][quads] each
    dt = x.dtype.type
    t0, t1 = d[4] - dt(4) * d[2], d[3] - dt(4) * d[1]
    t2, t3 = d[4] - d[2], d[3] - d[1]
    V = [dt(4) * d[0] + (d[4] - dt(5) * d[2]), t0 + t1, t0 - t1, t2 + dt(2) * t3, t2 - dt(2) * t3, dt(4) * d[1] + (d[5] - dt(5) * d[3])]
    U = [u.astype(x.dtype) for u in (f43_weights(w) if U is None else U)]
    m = [U[p] @ V[p] for p in range(6)]
    s12, d12, s34, d34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    y = np.zeros((cout, Tq), x.dtype)
    y[:, q0] = (m[0] + s12) + s34
    y[:, q0 + 1] = d12 + dt(2) * d34
    y[:, q0 + 2] = s12 + dt(4) * s34
    y[:, q0 + 3] = (d12 + dt(8) * d34) + m[5]
    return y[:, :T]


# conv_xlq.hip: QTab<k> — per k the entries (kind, tap offset): F(4,3) groups of three taps (a tap beyond the kernel is zero), k = 7's seventh tap alone
# (k = 9: the FFT blocks' FFN conv, conv_xres.hip WQ instances — three groups; k = 5: the frame-level pitch predictor, conv_k5q.hip — two groups, the sixth tap zero)
F43_TAPS = {3: [("f43", 0)], 5: [("f43", 0), ("f43", 3)], 7: [("f43", 0), ("f43", 3), ("one", 6)], 9: [("f43", 0), ("f43", 3), ("f43", 6)],
            11: [("f43", 0), ("f43", 3), ("f43", 6), ("f43", 9)]}


def f43_tap_weights(w):
    """w [Cout][Cin][k] -> the transformed weights of every product of F43_TAPS[k], in the kernels' point order: six per tap group, then k = 7's single
    tap as (g, g/2, g/2, g) — in double."""
    k = w.shape[-1]
    wz = np.concatenate([w, np.zeros(w.shape[:-1] + (2,), w.dtype)], axis=-1)
    U = []
    for kind, o in F43_TAPS[k]:
        g = wz[..., o].astype(np.float64)
        U += f43_weights(wz[..., o:o + 3]) if kind == "f43" else [g, 0.5 * g, 0.5 * g, g]
    return U


def conv1d_f43_taps(x, w, U=None):
    """The k = 3 / 5 / 7 / 9 / 11, dilation-1, padding-(k-1)/2 conv through conv_xlq_kernel's (k = 9: conv_xres_kernel<WQ>'s) products (cm-tts_amd/csrc/conv_xlq.hip; weights as
    weight_pack.cpp: to_wino43_iter_fragments forms them): all tap groups into six transform-domain accumulators, one output transform.  U: the points'
    transformed weights [points][Cout][Cin] (unpack_weights of a packed stream) instead of f43_tap_weights(w)."""
    cout, cin, k = w.shape
    T = x.shape[1]
    Tq = -(-T // 4) * 4
    pad = (k - 1) // 2
    xp = np.pad(x, ((0, 0), (pad, Tq - T + pad + 2)))
    q0 = np.arange(0, Tq, 4)
    dt = x.dtype.type
    M = [np.zeros((cout, q0.size), x.dtype) for _ in range(6)]
    U = [u.astype(x.dtype) for u in (f43_tap_weights(w) if U is None else U)]
    n = 0
    for kind, o in F43_TAPS[k]:
        if kind == "f43":
            d = [xp[:, q0 + o + i] for i in range(6)]
            t0, t1 = d[4] - dt(4) * d[2], d[3] - dt(4) * d[1]
            t2, t3 = d[4] - d[2], d[3] - d[1]
            V = [dt(4) * d[0] + (d[4] - dt(5) * d[2]), t0 + t1, t0 - t1, t2 + dt(2) * t3, t2 - dt(2) * t3, dt(4) * d[1] + (d[5] - dt(5) * d[3])]
            for p in range(6):
                M[p] = M[p] + U[n + p] @ V[p]
            n += 6
        else:
            xs = [xp[:, q0 + o + i] for i in range(4)]
            for i, (p, v) in enumerate(zip((0, 1, 2, 5), (xs[0] - xs[2], xs[1] + xs[2], xs[2] - xs[1], xs[3] - xs[1]))):
                M[p] = M[p] + U[n + i] @ v
            n += 4
    s12, d12, s34, d34 = M[1] + M[2], M[1] - M[2], M[3] + M[4], M[3] - M[4]
    y = np.zeros((cout, Tq), x.dtype)
    y[:, q0] = (M[0] + s12) + s34
    y[:, q0 + 1] = d12 + dt(2) * d34
    y[:, q0 + 2] = s12 + dt(4) * s34
    y[:, q0 + 3] = (d12 + dt(8) * d34) + M[5]
    return y[:, :T]


def conv1d_f43_taps_dil(x, w, dil=1, U=None):
    """conv_xlq_kernel at dilation 3 / 5 (conv_xlq.hip: residue classes): the outputs t = r (mod dil) are the UNDILATED same-padded conv on the class's
    subsequence x[:, r::dil], so every class goes through conv1d_f43_taps on its own.  A tile holds 60 / dil = 20 or 12 entries per class, both
    multiples of four and tiles start at multiples of 60: the kernel's quads are the subsequence's quads (entries 4 m .. 4 m + 3 of the class)."""
    if dil == 1:
        return conv1d_f43_taps(x, w, U)
    y = np.zeros((w.shape[0], x.shape[1]), x.dtype)
    U = f43_tap_weights(w) if U is None else U          # formed once for all classes
    for r in range(min(dil, x.shape[1])):
        y[:, r::dil] = conv1d_f43_taps(np.ascontiguousarray(x[:, r::dil]), w, U)
    return y


def pair_f43(x, w1, b1, w2, b2, dil, slope, U1=None, U2=None):
    """A k = 3 ResBlock pair as the chain of two conv_xlq launches in their own products: xt = conv1(leaky(x)) + b1 at dilation dil (residue classes),
    y = (conv2(leaky(xt)) + b2) + x at dilation 1 -> (y, xt), every operation in x's dtype.  conv_xlq_pair3_kernel forms the same products on conv1
    quads that start one frame earlier (its tile's xt covers [t0 - 1, ..)): fp32 Winograd rounding apart from this chain, not a bit-for-bit twin."""
    dt = x.dtype.type
    act = lambda v: np.where(v > 0, v, v * dt(slope))
    xt = conv1d_f43_taps_dil(act(x), w1, dil, U1) + b1.astype(x.dtype)[:, None]
    y = (conv1d_f43_taps(act(xt), w2, U2) + b2.astype(x.dtype)[:, None]) + x
    return y, xt


# ---- the host-side weight packers (cm-tts_amd/csrc/weight_pack.cpp) as index expressions.  p: k-major weights [taps][K][M] (P[tap][input channel][output row]),
# float32.  A stream is values[t, k, row] gathered over the layout's dimensions, t = the tap (plain layouts) or the transformed weight (Winograd layouts).
WINO_PAD_HG, WINO43_PAD_KS = 4, 4


def _grid(*dims):
    return np.meshgrid(*[np.arange(d) for d in dims], indexing="ij", sparse=True)


def _k32(base, l, j):          # v_mfma_f32_32x32x2_f32: lane l supplies A[m = l & 31][k = l >> 5]; element j = k-step j
    return base + 2 * j + (l >> 5)


def _k16(ks, l):               # v_mfma_f32_16x16x4_f32: lane l supplies A[m = l & 15][k = l >> 4]
    return 4 * ks + (l >> 4)


def frag_index(layout, taps, K, M):
    """layout -> (shape, t, k, row): the stream's dimensions (padding excluded) and, broadcast over them, which value each element holds."""
    if layout == "fragment_order":               # [taps][K/8][M/32][64 lanes][4]
        shape = (taps, K // 8, M // 32, 64, 4)
        t, g, mt, l, j = _grid(*shape)
        return shape, t, _k32(8 * g, l, j), 32 * mt + (l & 31)
    if layout == "fragment_iter_order":          # [K/16][taps][2][M/32][64 lanes][4]
        shape = (K // 16, taps, 2, M // 32, 64, 4)
        c, t, h, mt, l, j = _grid(*shape)
        return shape, t, _k32(16 * c + 8 * h, l, j), 32 * mt + (l & 31)
    if layout == "fragment16":                   # [taps][K/16][M/32][64 lanes][8]
        shape = (taps, K // 16, M // 32, 64, 8)
        t, g, mt, l, j = _grid(*shape)
        return shape, t, 16 * g + 8 * (l >> 5) + j, 32 * mt + (l & 31)
    if layout == "fragment16_iter":              # [K/32][taps][2][M/32][64 lanes][8]
        shape = (K // 32, taps, 2, M // 32, 64, 8)
        c, t, h, mt, l, j = _grid(*shape)
        return shape, t, 32 * c + 16 * h + 8 * (l >> 5) + j, 32 * mt + (l & 31)
    if layout == "wino_fragments":               # [K/4 half-groups][M/32][2][64 lanes][4]: transform 2 ps + (q >> 1)
        shape = (K // 4, M // 32, 2, 64, 4)
        hg, mt, ps, l, q = _grid(*shape)
        return shape, 2 * ps + (q >> 1), _k32(4 * hg, l, q & 1), 32 * mt + (l & 31)
    if layout == "wino_iter_fragments":          # [K/16][entries][2][M/32][64 lanes][4]
        shape = (K // 16, len(WINO_TAB[taps]), 2, M // 32, 64, 4)
        c, e, h, mt, l, j = _grid(*shape)
        return shape, e, _k32(16 * c + 8 * h, l, j), 32 * mt + (l & 31)
    if layout in ("wino43_fragments", "wino43_iter_fragments"):      # [K/4 k-steps][M/64 waves][points][64 lanes][4]
        shape = (K // 4, M // 64, sum(6 if kind == "f43" else 4 for kind, _ in F43_TAPS[taps]), 64, 4)
        ks, w, pt, l, i = _grid(*shape)
        return shape, pt, _k16(ks, l), 64 * w + 16 * i + (l & 15)
    if layout == "wino43_xres_fragments":        # [K/4][M/32][9][64 lanes][4]: element (pt & 1) * 2 + i of vector pt / 2
        shape = (K // 4, M // 32, 9, 64, 4)
        ks, mt, v, l, e = _grid(*shape)
        return shape, 2 * v + (e >> 1), _k16(ks, l), 32 * mt + 16 * (e & 1) + (l & 15)
    if layout == "wino23_xres_fragments":        # [K/4][M/32][3 tap groups][2][64 lanes][4]: element (tr & 1) * 2 + i of vector tr / 2
        shape = (K // 4, M // 32, 3, 2, 64, 4)
        ks, mt, grp, v, l, e = _grid(*shape)
        return shape, 4 * grp + 2 * v + (e >> 1), _k16(ks, l), 32 * mt + 16 * (e & 1) + (l & 15)
    raise KeyError(layout)


def frag_values(layout, p):
    """The values [t][K][M] a layout permutes: the taps themselves, or the transformed weights (formed in double, rounded to float32 once)."""
    if not layout.startswith("wino"):
        return p
    g = np.moveaxis(p, 0, -1).astype(np.float64)          # [K][M][taps]
    taps = p.shape[0]
    if layout == "wino_fragments":
        U = [wino_weight(g, kind, 0) for kind in range(4)]
    elif layout == "wino_iter_fragments":
        U = [wino_weight(g, kind, tau) for _, _, _, _, kind, tau in WINO_TAB[taps]]
    elif layout == "wino23_xres_fragments":
        U = [wino_weight(g, tr, tau) for tau in (0, 3, 6) for tr in range(4)]
    else:
        U = f43_tap_weights(g)
    return np.stack(U).astype(np.float32)


def cvt16(a, mode):
    """float32 -> the 16-bit patterns of weight_pack.cpp: host_cvt16 (mode 1 = bf16, round to nearest even on the bit pattern; 2 = fp16)."""
    if mode == 2:
        return a.astype(np.float16).view(np.uint16)
    u = a.view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def pack_weights(layout, p, mode=0):
    """p [taps][K][M] float32 -> the packed stream (float32, or uint16 for the fragment16 layouts), padding included."""
    p = np.ascontiguousarray(p, np.float32)
    taps, K, M = p.shape
    if layout == "fragment16_split":            # hi = fp16(w) fragments, then lo = fp16(w - hi) fragments
        hi = p.astype(np.float16).astype(np.float32)
        return np.concatenate([pack_weights("fragment16", hi, 2), pack_weights("fragment16", p - hi, 2)])
    _, t, k, row = frag_index(layout, taps, K, M)
    s = frag_values(layout, p)[t, k, row].ravel()
    if layout.startswith("fragment16"):
        return cvt16(s, mode)
    pad = {"wino_fragments": WINO_PAD_HG * (M // 32) * 2 * 256, "wino43_fragments": WINO43_PAD_KS * (M // 64) * 6 * 256}.get(layout, 0)
    return np.concatenate([s, np.zeros(pad, np.float32)])


def unpack_weights(layout, stream, taps, K, M):
    """The inverse index map: a packed float32 stream -> the values it holds as [t][Cout][Cin] (t = tap or transformed weight)."""
    shape, t, k, row = frag_index(layout, taps, K, M)
    n = int(np.prod(shape))
    U = np.full((int(t.max()) + 1, K, M), np.nan, np.float32)
    U[t, k, row] = np.asarray(stream[:n], np.float32).reshape(shape)
    assert not np.isnan(U).any()
    return np.ascontiguousarray(U.transpose(0, 2, 1))
