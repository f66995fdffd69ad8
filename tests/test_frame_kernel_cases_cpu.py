"""CPU checks of tests/frame_kernel_cases.py: the float64 definitions ARE the oracle's operations, the cases have the properties
tests/test_gpu_frame_kernels.py relies on, at most 1 % of an integer-stage case sits on a rounding boundary, and every check_* raises on a
result computed from a deliberately wrong definition (nothing is mutated in the library)."""
import numpy as np
import pytest

from oracle import cmtts_oracle as O
import frame_kernel_cases as FC
import text_kernel_cases as TC


def _close64(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-12 * max(np.abs(np.asarray(b)).max(), 1e-300)


def _ulps32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float((np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max())


# ----------------------------------------------------------------------------------------------------------------- definitions == oracle

def test_head_definitions_are_the_oracles():
    """layernorm_def / ln_linear_def / chan_linear_def == O.layer_norm + O.linear (time-major), float64 to 1e-12."""
    c = FC.head_case(65, 68, "relu", "none", 11)
    x = np.transpose(c["x"][:, :, :65], (0, 2, 1)).astype(np.float64)
    with O.precision("f64"):
        h = O.layer_norm(x, c["g"].astype(np.float64), c["be"].astype(np.float64), c["eps"])
        assert _close64(np.transpose(FC.layernorm_def(c["x"][:, :, :65], c["g"], c["be"], c["eps"], np.float64), (0, 2, 1)), h)
        assert _close64(FC.ln_linear_def(c, np.float64), O.linear(h, c["W"].astype(np.float64), c["bias"].astype(np.float64)))
        assert _close64(FC.chan_linear_def(c, np.float64), O.linear(x, c["W"].astype(np.float64), c["bias"].astype(np.float64)))
    # masks: a column masked by ln_lens enters the linear as 0 (-> the bias), a position masked by out_lens is 0
    m = FC.head_case(65, 68, "relu", "differ", 11)
    out = FC.ln_linear_def(m, np.float64)
    assert not out[0, int(m["out_lens"][0]):].any()
    assert np.array_equal(out[2, 1:], np.broadcast_to(m["bias"].astype(np.float64), out[2, 1:].shape))


def test_integer_definitions_are_the_oracles():
    rs = np.random.RandomState(0)
    v = rs.uniform(-3, 3, 400).astype(np.float32)
    bins, _ = FC.energy_tables()
    assert np.array_equal(FC.bucketize_def(v, bins), O.bucketize(v, bins))
    for ctl in FC.DUR_CONTROLS:
        c = FC.dur_case(200, "spread", ctl)
        for prec, dt in (("f64", np.float64), ("f32", np.float32)):
            with O.precision(prec):
                assert np.array_equal(FC.durations_def(c["logd"], np.float32(ctl), dt)[1], O.durations_from_log(c["logd"], np.float32(ctl)))
    # integer durations: cumsum_def + mel2ph_def == dur_to_mel2ph, and the gather == length_regulate
    dur = rs.randint(0, 5, (3, 37)).astype(np.float32)
    cum, ml = FC.cumsum_def(dur)
    assert np.array_equal(FC.mel2ph_def(cum, 90), O.dur_to_mel2ph(dur, np.zeros(dur.shape, bool), 90))
    g = FC.gather_case(257)
    dur2 = np.diff(np.concatenate([np.zeros((3, 1), np.int64), FC.frames_case(257, FC.GATHER_L, (257, 154, 0), 21)[0].astype(np.int64)], 1), axis=1)
    ref, _ = O.length_regulate(np.transpose(g["out1"][:, :, :FC.GATHER_L], (0, 2, 1)), dur2, 257)
    assert np.array_equal(FC.length_regulate_def(g), np.transpose(ref, (0, 2, 1)))


def test_pitch_definition_is_the_oracles():
    from cmtts_amd.config import get_config
    cfg = get_config("LJSpeech")
    assert cfg.pitch_norm_eps == FC.PITCH_EPS and cfg.use_uv
    c = FC.pitch_case(257, 11, 1, 1.3)
    for prec, dt in (("f64", np.float64), ("f32", np.float32)):
        with O.precision(prec):
            std = c["std"].astype(dt) * dt(np.float32(c["std_scale"]))
            idx, f0d, _ = O.cwt_to_pitch_index(c["cwt"].astype(dt), c["mean"].astype(dt), std, cfg)
        _, mine_f0, mine_idx = FC.pitch_def(c, dt)
        if dt is np.float64:
            assert _close64(mine_f0, f0d) and np.array_equal(mine_idx, idx)
        else:
            assert _ulps32(mine_f0, f0d) <= 4


def test_position_definitions_are_the_oracles():
    c = FC.pos_case(257)
    flags = c["x"][:, 0, :257] != 0
    assert np.array_equal(FC.positions_def(flags), O.make_positions(flags))
    # the oracle's table takes sin / cos in fp32; the kernel's recipe (float64 sine of the fp32 product, rounded) is within an ulp of 1 of it
    pe = FC.pos_embed(FC.positions_def(flags), FC.POS_C)
    assert np.abs(pe - O.positional_embedding(c["x"][:, 0, :257], FC.POS_C)).max() <= 2 * np.spacing(np.float32(1))
    assert np.array_equal(FC.pos_table(100, FC.POS_C), FC.pos_embed(np.arange(100), FC.POS_C)) and not FC.pos_table(100, FC.POS_C)[0].any()


def test_dense_and_conv_definitions_are_the_oracles():
    v = np.linspace(-30, 30, 601)
    with O.precision("f64"):
        assert _close64(FC.mish_def(v, np.float64), O.mish(v))
        assert _close64(TC.gelu(v), O.gelu_erf(v))
    assert _ulps32(FC.mish_def(v.astype(np.float32), np.float32), O.mish(v.astype(np.float32))) <= 4
    # the generic conv's definition on a plain case == O.conv1d; the transposed-conv phases == O.conv_transpose1d
    c = FC.conv_case("t64x256", 257)
    a, b = c["a"], c["bufs"]
    w = np.transpose(b["A"][0][:, :, :a["M"]], (2, 1, 0)).astype(np.float64)
    x = b["X"][:, :, :a["Tin"]].astype(np.float64)
    x = np.where(x > 0, x, x * np.float64(np.float32(0.1)))
    with O.precision("f64"):
        ref = O.conv1d(x, w, b["bias"].astype(np.float64), padding=a["pad"], dilation=a["dil"])
    ys, wr = FC.conv_def(c, np.float64)
    got = ys["Y0"].reshape(b["Y0"].shape)
    assert _close64(got[:, :, :257], ref) and (got[:, :, 257:] == FC.SENTINEL).all() and wr["Y0"].reshape(b["Y0"].shape)[:, :, :257].all()
    t = FC.conv_case("convT", 256)
    tb = t["bufs"]
    x = tb["X"].astype(np.float64) / 3.0
    with O.precision("f64"):
        ref = O.conv_transpose1d(np.where(x > 0, x, x * np.float64(np.float32(0.1))), tb["W"].astype(np.float64), tb["bias"].astype(np.float64), 4, 2)
    assert _close64(FC.conv_transpose_def(t, np.float64), ref)
    ys, wr = FC.conv_def(t, np.float64)
    assert wr["Y0"].all() and _close64(ys["Y0"].reshape(ref.shape), ref)


# ----------------------------------------------------------------------------------------------------------------- properties of the cases

def test_lengths_fall_inside_tiles():
    for T in FC.HEAD_T + FC.POS_T + FC.SOFTMAX_L:
        lens = FC.case_lens(T)
        assert lens[0] == T and lens[2] == 1 and 1 <= lens[1] <= T
        if T > 2:
            assert lens[1] % 16 != 0 and lens[1] < T
    for T in FC.HEAD_T:
        for ld in FC.head_lds(T):
            assert ld % 4 == 0 and ld >= T
    assert FC.head_lds(17) == (20, 28) and FC.head_lds(65) == (68, 76) and FC.head_lds(64) == (64,)


def test_head_regimes():
    c = FC.head_case(130, 132, "offset")
    x = c["x"][:, :, :130].astype(np.float64)
    assert (x.var(1) / x.mean(1) ** 2).max() < 1e-5                       # the one-pass variance's regime
    d = FC.head_case(130, 132, "dead")
    col = d["x"][:, :, 65]
    assert (col == FC.DEAD_VALUE).all()
    for dt in (np.float32, np.float64):                                   # exactly beta, finite, in both evaluations
        h = FC.layernorm_def(d["x"][:, :, :130], d["g"], d["be"], d["eps"], dt)
        assert np.array_equal(h[:, :, 65], np.broadcast_to(d["be"].astype(dt), (3, 256))) and np.isfinite(h).all()
    assert (FC.head_case(130, 132, "relu")["x"][:, :, :130] >= 0).all()
    assert (np.abs(c["x"][:, :, 130:]) == FC.GARBAGE).all()


def test_energy_targets_sit_on_edges():
    c = FC.energy_case(130, 132, "target")
    bins, tg = c["bins"], c["e_target"].reshape(-1)
    assert np.isin(tg[0::5], bins).all() and np.isnan(tg[1]) and tg[2] < bins[0] and tg[3] > bins[-1] and tg[6] == bins[-1]
    idx = FC.energy_def(c, np.float64)[2].reshape(-1)
    assert idx[1] == FC.NBINS and idx[2] == 0 and idx[3] == FC.NBINS and idx[6] == FC.NBINS - 1
    assert (bins[idx[0::5]] == tg[0::5]).all()                            # side = 'left': the edge's own bucket


def test_integer_stage_cases_stay_off_boundaries():
    """At most 1 % of the elements of EVERY integer-stage case the GPU test runs lie within the project's margin (test_gpu_text_kernels.DUR_MARGIN,
    ENERGY_MARGIN, conftest.FLIP_MARGIN) of a boundary of the float64 pre-rounding value; this module's own margins do not exceed them; the
    clear duration set is at least 0.2 from a boundary."""
    import test_gpu_text_kernels as G
    from conftest import FLIP_MARGIN
    assert FC.FRAME_DUR_MARGIN <= G.DUR_MARGIN and FC.FRAME_ENERGY_MARGIN <= G.ENERGY_MARGIN and FC.FRAME_PITCH_MARGIN <= FLIP_MARGIN
    for L in FC.DUR_L:
        for kind, ctl, table, B in FC.dur_cases(L):
            c = FC.dur_case(L, kind, ctl, table, B)
            u = FC.durations_def(c["logd"], FC.dur_ctl(c), np.float64)[0]
            assert (TC.half_margin(u) < G.DUR_MARGIN).sum() <= 0.01 * u.size, (L, kind, ctl, table, B)
            if kind == "clear":
                assert TC.half_margin(u).min() >= 0.2
    for T, ld, mode in FC.energy_cases():
        if mode != "target":          # (targets sit on edges on purpose and are bucketized exactly)
            c = FC.energy_case(T, ld, mode)
            v = FC.energy_def(c, np.float64)[1]
            assert (TC.int_margin(TC.energy_units(v, c["bins"])) < G.ENERGY_MARGIN).sum() <= 0.01 * v.size, (T, ld, mode)
    for T in FC.PITCH_T:
        for O, stat_ld, std_scale in FC.PITCH_COMBOS:
            c = FC.pitch_case(T, O, stat_ld, std_scale)
            _, f0, idx = FC.pitch_def(c, np.float64)
            assert (~FC.pitch_margin_mask(f0, FLIP_MARGIN)).sum() <= 0.01 * f0.size, (T, O, stat_ld, std_scale)
            if T >= 255:
                assert idx[:2].min() == 1 and idx[:2].max() >= 250 and (idx[2][~FC.unvoiced(c)[2]] == 255).all()


def test_duration_cases():
    c = FC.dur_case(200, "spread")
    ld = c["logd"]
    assert np.abs(ld).max() <= 6 and (ld == 0).any() and (np.exp(ld.astype(np.float64)) - 1 < -0.5).any()
    assert np.trunc(FC.durations_def(ld, np.float32(1), np.float64)[1][:, :64]).sum(1).min() > 64 * 15       # a large carry into the second lane group
    assert FC.dur_case(200, "spread", 1.0, None, 65)["logd"].shape == (65, 200)
    k = FC.dur_case(129, "spread", 0.5, "const")
    assert (k["table"] == np.float32(0.5)).all()
    d = FC.durations_def(k["logd"], k["table"], np.float64)[1]
    assert (d % 1 == 0.5).any()                                           # truncation and rint differ here


def test_cumsum_and_frames_cases():
    for L in FC.CUM_L:
        for scale, tg in FC.CUM_SCALES.items():
            c = FC.cumsum_case(L, scale)
            cum, ml = FC.cumsum_def(c["dur"])
            assert tuple(ml) == tg and (c["dur"] % 1 != 0).any()
            if L >= 64:
                assert (c["dur"] < 0).any() and (np.diff(cum, axis=1) == 0).any()
    assert min(FC.CUM_T) < 3 < 120 < 255 and 200 < 255 and 256 in FC.CUM_T and 257 < 400
    c = FC.pitch_table_case(257)
    assert tuple(c["cum"][:, -1]) == (257, 294, 0, 128)
    assert (FC.gather_case(257)["mel2ph"] == 0).any() and FC.GATHER_LDL != FC.GATHER_L


def test_position_cases():
    for T in FC.POS_T:
        c = FC.pos_case(T)
        if T >= 3:
            x0 = c["x"][:, 0, :T]
            assert (x0[:, T // 3] == 0).all() and np.signbit(x0[:, T // 2]).all() and (x0[:, T // 2] == 0).all()
            assert c["lens"][1] < T
        for z in (True, False):
            p = FC.pos_lr_case(T, z)
            assert (p["padv"][0] == 0) == z
        e = FC.embed_case(T)
        if T >= 3:
            assert e["texts"][0, T // 2] == 0 and (e["texts"][1, int(e["lens"][1]):] != 0).all()
    # an off-by-one position moves the output by far more than any bound: channel 0 is sin(p), omega_0 = 1
    assert FC.pos_omega(FC.POS_C)[0] == 1 and FC.POS_ALPHA * abs(np.sin(5.0) - np.sin(6.0)) > 0.5
    assert max(FC.POS_T) < FC.POS_TAB_ROWS[-1] and 0 < FC.POS_TAB_ROWS[1] < 255


def test_dense_cases_select_their_kernels():
    """k_dense_small: dense_small_kernel<16> when K >= 512 and ceil(N / 64) x ceil(B / 8) < 128 workgroups, else <4>; k_stats_mlp declines when
    (K0 + N0 + N1 + 3 x 128) floats exceed 48 KB; k_conv_post takes the 16-byte-load kernel only with ld % 4 == 0, ld >= T rounded up to 4, T >= 4."""
    assert FC.dense_slices(8, 1024, 64) == 16 and FC.dense_slices(9, 256, 130) == 4 and FC.dense_slices(1, 3, 1) == 4
    assert all(FC.dense_slices(B, 1024, N) == 16 for B in FC.DENSE_B for N in FC.DENSE_N)
    pre = FC.dense_def(FC.dense_case(9, 256, 130), np.float64, FC.DENSE_NONE, True, False)
    assert pre.min() < -25 and pre.max() > 25          # both sides of Mish's v > 20 branch, down to where log1p(exp(v)) underflows
    for s in FC.STATS_SHAPES:
        assert FC.stats_lds_bytes(*s[:3]) <= 48 * 1024
    assert FC.stats_lds_bytes(*FC.STATS_DECLINED[:3]) > 48 * 1024 and FC.STATS_SHAPES[0][1] % 128 and FC.STATS_SHAPES[0][2] % 128
    assert FC.post_takes_v4(1029, 1032, 7) and not FC.post_takes_v4(1029, 1030, 7) and not FC.post_takes_v4(3, 4, 7) and FC.post_takes_v4(4, 4, 3)


def test_conv_cases_select_their_configurations():
    """cmtts_launch_conv (conv_mfma.hip), restated in frame_kernel_cases.conv_config: gated -> 128 x 128 (M % 64 == 0); M > 64: a split
    (multiple of 128) -> 128 x 128, else below 512 128 x 128 tiles -> 64 x 64 with 64-channel chunks (one tap, K >= 128), five taps per
    barrier (taps > 1) or plain; M <= 64: one tap, K >= 128 and fewer than 256 column tiles -> 64 x 64 / 64-channel chunks, else 64 x 256
    (M > 32) or 32 x 256; a halo above 64, a split on M <= 64, a split off 128 and a gated M off 64 are refused."""
    for config in FC.CONV_CONFIGS:
        tile = FC.CONV_TILE_N[config]
        for N in (2 if config == "convT" else 1, tile - 1, tile, tile + 1):
            c = FC.conv_case(config, N)
            assert FC.conv_config(c["a"], c["epi"], c["nbatch"]) == FC.CONV_EXPECT[config], (config, N)
            assert tile == FC.CONV_EXPECT[config][1]
    a = dict(FC.conv_case("gated", 128)["a"], M=96)
    assert FC.conv_config(a, FC.EPI_GATED, 2) == -2
    a = dict(FC.conv_case("split", 128)["a"], split=64)
    assert FC.conv_config(a, FC.EPI_PLAIN, 2) == -2
    a = dict(FC.conv_case("tb5", 64)["a"], dil=9)
    assert FC.conv_config(a, FC.EPI_PLAIN, 2) == -2
    assert FC.conv_case("kc64", 64, 1)["a"]["Tin"] < 64


# ----------------------------------------------------------------------------------------------------------------- every check can fail

def _raises(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_checks_pass_on_the_float32_definition_and_fail_on_mutants():
    # one-pass variance in the offset regime
    c = FC.head_case(130, 132, "offset", "none", 11)
    FC.check_ln_linear(FC.ln_linear_def(c, np.float32), c)
    with np.errstate(all="ignore"):
        _raises(FC.check_ln_linear, FC.ln_linear_def(c, np.float32, one_pass=True), c)
        x = c["x"][:, :, :130]
        FC.check_layernorm(FC.layernorm_def(x, c["g"], c["be"], c["eps"], np.float32), c)
        _raises(FC.check_layernorm, FC.layernorm_def(x, c["g"], c["be"], c["eps"], np.float32, one_pass=True), c)
    # a masked column that keeps beta instead of 0
    m = FC.head_case(65, 68, "relu", "differ", 10)
    FC.check_ln_linear(FC.ln_linear_def(m, np.float32), m)
    _raises(FC.check_ln_linear, FC.ln_linear_def(m, np.float32, masked_keeps_beta=True), m)
    FC.check_chan_linear(FC.chan_linear_def(m, np.float32), m)


def _energy_result(c, side="left"):
    pred, v, idx = FC.energy_def(c, np.float32, side)
    out1 = np.zeros_like(c["xin"])
    out1[:, :, :c["T"]] = c["xin"][:, :, :c["T"]] + np.transpose(c["E"][idx], (0, 2, 1))
    es = v.astype(np.float32) if (c["e_table"] is not None or (c["e_control"] != 1.0 and c["e_target"] is None)) else np.full(v.shape, FC.SENTINEL, np.float32)
    return {"out": pred[:, :, None], "e_idx": idx, "out1": out1, "e_scaled": es}


def test_energy_check_fails_on_right_sided_bucketize():
    for mode in FC.ENERGY_MODES:
        c = FC.energy_case(65, 76, mode)
        FC.check_energy(_energy_result(c), c)
    c = FC.energy_case(65, 76, "target")
    _raises(FC.check_energy, _energy_result(c, "right"), c)
    bad = _energy_result(FC.energy_case(65, 76, "ctl1"))
    bad["e_scaled"] = bad["out"][:, :, 0].copy()
    _raises(FC.check_energy, bad, FC.energy_case(65, 76, "ctl1"))


def _dur_result(c, dtype=np.float32, cum_round=np.trunc):
    _, d, cum, ml = FC.durations_def(c["logd"], FC.dur_ctl(c), dtype, cum_round)
    return {"d_rounded": d.astype(np.float32), "cum": cum.astype(np.int32), "mel_len": ml}


def test_duration_check_fails_on_rint_and_on_a_dropped_carry():
    for kind in FC.DUR_KINDS:
        for ctl in FC.DUR_CONTROLS:
            c = FC.dur_case(129, kind, ctl)
            FC.check_durations(_dur_result(c), c)
    c = FC.dur_case(129, "spread", 0.5)
    _raises(FC.check_durations, _dur_result(c, cum_round=np.rint), c)
    bad = _dur_result(c)
    bad["cum"] = bad["cum"].copy()
    bad["cum"][:, 64:] -= bad["cum"][:, 63:64]                             # the carry into the second lane group dropped
    _raises(FC.check_durations, bad, c)
    # a duration that differs from float64 away from a boundary
    bad = _dur_result(FC.dur_case(129, "clear"))
    bad["d_rounded"] = bad["d_rounded"] + 1
    bad["cum"] = np.cumsum(bad["d_rounded"].astype(np.int64), 1).astype(np.int32)
    bad["mel_len"] = bad["cum"][:, -1].astype(np.int64)
    _raises(FC.check_durations, bad, FC.dur_case(129, "clear"))
    cs = FC.cumsum_case(64)
    cum, ml = FC.cumsum_def(cs["dur"])
    FC.check_cumsum({"cum": cum, "mel_len": ml}, cs)
    _raises(FC.check_cumsum, {"cum": np.cumsum(np.rint(cs["dur"]).astype(np.int64), 1), "mel_len": ml}, cs)
    FC.check_mel2ph(FC.mel2ph_def(cum, 257), cs, 257)
    _raises(FC.check_mel2ph, np.maximum(FC.mel2ph_def(cum, 257) - 1, 0), cs, 257)


def _pitch_result(c, **kw):
    r, f0, idx = FC.pitch_def(c, np.float32, **kw)
    return {"r_ws": r, "f0_denorm": f0, "p_idx": idx}


def test_pitch_check_fails_on_biased_deviation_and_on_uv_ge():
    for T in (3, 700):
        c = FC.pitch_case(T, 11, 2, 1.3)
        FC.check_pitch(_pitch_result(c), c)
        _raises(FC.check_pitch, _pitch_result(c, ddof=0), c)
        _raises(FC.check_pitch, _pitch_result(c, uv_ge=True), c)
    c = FC.pitch_case(257, 10, 1, 1.0)
    FC.check_pitch(_pitch_result(c), c)
    p = FC.pitch_table_case(257)
    FC.check_pitch_table(FC.pitch_table_def(p), p)
    _raises(FC.check_pitch_table, p["cwt"], p)


def test_position_checks_fail_on_positions_that_do_not_skip():
    c = FC.pos_case(257)
    FC.check_pos_embed_add(FC.pos_embed_add_def(c, np.float32, True), c, True)
    _raises(FC.check_pos_embed_add, FC.pos_embed_add_def(c, np.float32, False, skip=False), c, False)
    p = FC.pos_lr_case(257, True)
    FC.check_pos_embed_add_lr(FC.pos_embed_add_lr_def(p, np.float32), p)
    _raises(FC.check_pos_embed_add_lr, FC.pos_embed_add_lr_def(p, np.float32, skip=False), p)
    e = FC.embed_case(257)
    FC.check_embed_tokens(FC.embed_tokens_def(e, np.float32), e)
    _raises(FC.check_embed_tokens, FC.embed_tokens_def(e, np.float32, skip=False), e)
    g = FC.gather_case(257)
    FC.check_length_regulate(FC.length_regulate_def(g, g["padv"]), g, True)
    _raises(FC.check_length_regulate, FC.length_regulate_def(g), g, True)


def test_small_dense_checks():
    c = FC.dense_case(9, 255, 65, 3)
    for act in (FC.DENSE_NONE, FC.DENSE_RELU, FC.DENSE_MISH):
        FC.check_dense(FC.dense_def(c, np.float32, act, True, True), c, act, True, True)
    _raises(FC.check_dense, FC.dense_def(c, np.float32, FC.DENSE_RELU, True, True), c, FC.DENSE_MISH, True, True)
    s = FC.stats_case(FC.STATS_SHAPES[0])
    FC.check_stats_mlp(FC.stats_def(s, np.float32), s)
    for regime in FC.SOFTMAX_REGIMES:
        m = FC.softmax_case(65, regime)
        FC.check_softmax(FC.softmax_def(m, np.float32), m)
    bad = FC.softmax_def(m, np.float32)
    bad[2, -1] = 1e-30                                                     # a masked key that is not exactly 0
    _raises(FC.check_softmax, bad, m)
    r = FC.reduce_case(6, 65)
    FC.check_reduce(FC.reduce_def(r, np.float32, True, True, True), r, True, True, True)
    _raises(FC.check_reduce, FC.reduce_def(r, np.float64, True, True, True).astype(np.float32), r, True, True, True)      # pairwise / wider sums differ in bits
    p = FC.post_case(1029, 30, 7, 1032)
    FC.check_conv_post(FC.conv_post_def(p, np.float32), p)
    _raises(FC.check_conv_post, FC.conv_post_def(p, np.float32)[:, ::-1], p)
    k = FC.mel_case(100)
    FC.check_mel_prep(FC.mel_prep_def(k, np.float32, True), k, True)
    FC.check_mel_post(FC.mel_post_def(k, np.float32, True, True), k, True, True)
    _raises(FC.check_mel_post, FC.mel_post_def(k, np.float32, True, False), k, True, True)
    rows = FC.mel_post_def(k, np.float32, True, True, k["rows"])
    out, fin = np.full_like(rows, FC.SENTINEL), np.full_like(rows, FC.SENTINEL)
    out[:2], fin[2] = rows[:2], rows[2]
    FC.check_mel_post_rows(out, fin, k, FC.SENTINEL)
    _raises(FC.check_mel_post_rows, rows, fin, k, FC.SENTINEL)
    FC.check_diff_embed(FC.diff_embed_def(k, np.float32), k)


def test_remaining_checks_fail_on_wrong_results():
    """The checks no mutant above reaches: rows of W swapped (chan_linear), a dropped ReLU (stats_mlp), the scalar scale where the per-utterance
    one is due (mel_prep), sine and cosine halves swapped (diff_embed), an embedding index shifted by one (lr_gather_add, gather_add)."""
    m = FC.head_case(65, 68, "relu", "same", 10)
    good = FC.chan_linear_def(m, np.float32)
    FC.check_chan_linear(good, m)
    _raises(FC.check_chan_linear, np.ascontiguousarray(good[:, :, ::-1]), m)
    keeps = good.copy()
    keeps[1, int(m["out_lens"][1])] = m["bias"]                            # a masked position that holds the bias instead of 0
    _raises(FC.check_chan_linear, keeps, m)
    s = FC.stats_case(FC.STATS_SHAPES[0])
    h = s["x"] @ s["W"][0] + s["b"][0]                                     # no ReLU behind the first layer
    h = np.maximum(h @ s["W"][1] + s["b"][1], 0)
    _raises(FC.check_stats_mlp, (h @ s["W"][2] + s["b"][2]).astype(np.float32), s)
    k = FC.mel_case(100)
    _raises(FC.check_mel_prep, FC.mel_prep_def(k, np.float32, False), k, True)
    emb = FC.diff_embed_def(k, np.float32)
    _raises(FC.check_diff_embed, np.roll(emb, FC.DIFF_C // 2, 1), k)
    g = FC.gather_case(257)
    shifted = np.transpose(g["E"][(g["idx"] + 1) % FC.GATHER_NE], (0, 2, 1))
    FC.check_lr_gather_add((FC.length_regulate_def(g) + np.transpose(g["E"][g["idx"]], (0, 2, 1))).astype(np.float32), g)
    _raises(FC.check_lr_gather_add, (FC.length_regulate_def(g) + shifted).astype(np.float32), g)
    FC.check_gather_add((g["x"] + np.transpose(g["E"][g["idx"]], (0, 2, 1))).astype(np.float32), g)
    _raises(FC.check_gather_add, (g["x"] + shifted).astype(np.float32), g)


def _conv_result(c, **kw):
    ys, _ = FC.conv_def(c, np.float32, **kw)
    return {k: v.astype(np.float32) for k, v in ys.items()}


def test_conv_check_fails_on_swapped_gate_ignored_row_off_and_shifted_phase():
    for config in FC.CONV_CONFIGS:
        c = FC.conv_case(config, FC.CONV_TILE_N[config] + 1)
        FC.check_conv(_conv_result(c), c)
    g = FC.conv_case("gated", 129)
    _raises(FC.check_conv, _conv_result(g, swap_gate=True), g)
    s = FC.conv_case("split", 129, 1)
    FC.check_conv(_conv_result(s), s)
    _raises(FC.check_conv, _conv_result(s, ignore_row_off=True), s)
    t = FC.conv_case("convT", 257)
    _raises(FC.check_conv, _conv_result(t, phase_shift=1), t)
