"""Seeded per-utterance sampler noise, the parts that need no GPU: the numpy statement of the definition (cmtts_amd/noise.py) against
the published Philox4x32-10 / splitmix64 vectors and the worked examples of DESIGN.md §3.6c, its prefix / window properties, its
moments, the "determ-indiv" generator's index rule, and the argument checks and bindings of the new C entry points."""
import ctypes as C

import numpy as np
import pytest

from cmtts_amd import _lib, noise

SEED = 0xE9D83B46B561CAF5


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert _hex(noise.philox4x32_10(np.asarray(ctr, np.uint32), np.asarray(key, np.uint32))) == want


def test_philox_broadcasts():
    ctr = np.zeros((3, 2, 4), np.uint32)
    ctr[1, 1] = 0xFFFFFFFF
    key = np.zeros((3, 2, 2), np.uint32)
    key[1, 1] = 0xFFFFFFFF
    out = noise.philox4x32_10(ctr, key)
    assert out.shape == (3, 2, 4) and out.dtype == np.uint32
    assert _hex(out[0, 0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(out[1, 1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_splitmix_and_utterance_seeds():
    assert noise.splitmix64(0) == 0xE220A8397B1DCDAF
    got = noise.utterance_seeds(1234, [0, 1, 7])
    assert got.dtype == np.int64
    assert [int(v) for v in got.view(np.uint64)] == [0x9E17E35F6D9238ED, 0xB2B8EC3A6254E62C, 0xE9D83B46B561CAF5]
    # an id is added mod 2^64: a negative id is its two's complement
    assert noise.utterance_seeds(1234, [-1])[0] == noise.utterance_seeds(1234, np.asarray([2 ** 64 - 1], np.uint64))[0]


def test_worked_examples():
    bits = noise.reference_bits(SEED, 1, 512, 80, first_draw=2)
    assert bits.shape == (1, 1, 512, 20, 4)
    assert _hex(bits[0, 0, 511, 19]) == "66be4ab8 a7cee491 851776fa 646dc015"          # block j = 511 * 20 + 19 = 10239
    z = noise.reference_normals(SEED, 1, 512, 80, first_draw=2)
    assert z.shape == (1, 1, 1, 512, 80) and z.dtype == np.float64
    assert np.abs(z[0, 0, 0, 511, 76:] - [-0.755997981, -1.119979478, -0.891755454, 0.716275770]).max() <= 1e-8
    z0 = noise.reference_normals(SEED, 1, 1, 80)
    assert np.abs(z0[0, 0, 0, 0, :4] - [0.546333918, -1.288766766, -1.449605070, -0.714283977]).max() <= 1e-8
    # the int64 form of the same seed is the same utterance
    assert np.array_equal(noise.reference_normals(np.asarray([SEED], np.uint64).view(np.int64), 1, 1, 80), z0)


def test_prefix_window_and_batch_properties():
    seeds = noise.utterance_seeds(7, np.arange(3))
    full = noise.reference_normals(seeds, 2, 100, 80)
    assert np.array_equal(full[:, :, :, :37], noise.reference_normals(seeds, 2, 37, 80))
    assert np.array_equal(full[:, :, :, 64:], noise.reference_normals(seeds, 2, 36, 80, t0=64))
    assert np.array_equal(full[1:], noise.reference_normals(seeds, 1, 100, 80, first_draw=1))
    assert np.array_equal(full[:, 1:2], noise.reference_normals(seeds[1:2], 2, 100, 80))
    assert np.array_equal(full[:, ::-1], noise.reference_normals(seeds[::-1], 2, 100, 80))
    # n_mels not a multiple of 4: the last block of a row is cut, rows do not share blocks
    z6 = noise.reference_normals(seeds, 1, 5, 6)
    b6 = noise.normals_from_bits(noise.reference_bits(seeds, 1, 5, 6))
    assert z6.shape == (1, 3, 1, 5, 6) and np.array_equal(z6[0, :, 0], b6[0].reshape(3, 5, 8)[..., :6])
    # frames beyond 2^32 blocks: the counter's second word takes over
    t0 = 214748365                          # j = 20 t0 + 3 = 2^32 + 7
    su = int(seeds.view(np.uint64)[0])
    want = noise.philox4x32_10(np.asarray([7, 1, 0, noise.COUNTER_TAG], np.uint32), np.asarray([su & 0xFFFFFFFF, su >> 32], np.uint32))
    assert np.array_equal(noise.reference_bits(seeds[:1], 1, 1, 80, t0=t0)[0, 0, 0, 3], want)
    assert np.abs(full).max() <= 5.77


def moment_z(z):
    """z-scores of the mean, the standard deviation and the fourth moment of n standard normal values."""
    z = np.asarray(z, np.float64).reshape(-1)
    n = z.size
    return np.sqrt(n) * z.mean(), np.sqrt(2 * n) * (z.std() - 1.0), ((z ** 4).mean() - 3.0) / np.sqrt(96.0 / n)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_moments(seed):
    z = noise.reference_normals(noise.utterance_seeds(seed, np.arange(8)), 5, 512, 80)
    zs = moment_z(z)
    print(f"NOISE moments (numpy), seed {seed}: z(mean) {zs[0]:+.2f} z(sd) {zs[1]:+.2f} z(m4) {zs[2]:+.2f} max|z| {np.abs(z).max():.2f}")
    assert all(abs(v) <= 4 for v in zs), zs
    assert np.abs(z).max() <= 5.78


def test_generator_index_rule():
    assert noise.indiv_indices(4, 100).tolist() == [0, 1, 2, 3]
    assert noise.indiv_indices(4, 100, done_samples=10, rank=1, world=3).tolist() == [11, 14, 17, 20]
    assert noise.indiv_indices(4, 16, done_samples=10, rank=1, world=3).tolist() == [11, 14, 15, 15]          # clamped to num_samples - 1
    # the ranks of a world cover a batch of world * n consecutive samples exactly once
    got = sorted(i for r in range(4) for i in noise.indiv_indices(5, 1000, 40, r, 4).tolist())
    assert got == list(range(40, 60))
    from cmtts_amd import host
    gen = host.get_generator("determ-indiv", 100, 3)
    assert isinstance(gen, host.IndivGenerator) and gen.get_seed() == 3 and (gen.rank, gen.world_size) == (0, 1)
    size, idx = gen.get_size_and_indices((4, 1, 9, 80))
    assert size == (1, 1, 9, 80) and idx.tolist() == [0, 1, 2, 3]
    gen.set_done_samples(98)
    assert gen.get_size_and_indices((4, 1, 9, 80))[1].tolist() == [98, 99, 99, 99]
    assert np.array_equal(gen.seeds_for(4), noise.utterance_seeds(3, [98, 99, 99, 99]))
    gen.set_seed(4)
    assert gen.get_seed() == 4 and np.array_equal(gen.seeds_for(1), noise.utterance_seeds(4, [98]))
    assert isinstance(host.get_generator("dummy"), host.DummyGenerator)
    with pytest.raises(NotImplementedError, match="num_samples"):
        host.get_generator("determ", 10, 0)
    with pytest.raises(NotImplementedError):
        host.get_generator("other")


def test_bindings_listed():
    for name in ("cmtts_noise_fill", "cmtts_noise_fill_groups", "cmtts_sample_seeded_workspace_bytes", "cmtts_sample_seeded"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cmtts_sample_seeded"][1]) == len(_lib.SIGNATURES["cmtts_sample_factored_t"][1])
    assert [n for n, _ in _lib.NoiseGroupStruct._fields_] == ["seeds", "B", "T", "out"]


def test_entry_points_reject_bad_arguments():
    """CMTTS_E_INVALID (-1) before any launch: the pointers below are never dereferenced."""
    lib = _lib.load()
    p, s = 0x1000, None          # a non-null "device pointer" that a rejected call never touches

    def fill(seeds=p, B=2, T=3, M=80, first=0, n=1, t0=0, out=p):
        return lib.cmtts_noise_fill(seeds, B, T, M, first, n, t0, out, s)

    bad = {"null seeds": fill(seeds=None), "null out": fill(out=None), "B": fill(B=0), "T": fill(T=0), "M": fill(M=0), "n_draws": fill(n=0),
           "B < 0": fill(B=-1), "first_draw": fill(first=-1), "t0": fill(t0=-1)}
    assert all(rc == -1 for rc in bad.values()), bad
    assert b"cmtts_noise_fill" in lib.cmtts_last_error()

    def groups(g=((p, 2, 3, p),), n=None, M=80, first=0, nd=1):
        arr = (_lib.NoiseGroupStruct * max(len(g), 1))()
        for a, (sd, B, T, out) in zip(arr, g):
            a.seeds, a.B, a.T, a.out = sd, B, T, out
        return lib.cmtts_noise_fill_groups(arr, len(g) if n is None else n, M, first, nd, s)

    bad = {"null table": lib.cmtts_noise_fill_groups(None, 1, 80, 0, 1, s), "n_groups": groups(n=0), "M": groups(M=0), "n_draws": groups(nd=0),
           "first_draw": groups(first=-1), "null seeds": groups(g=((None, 2, 3, p),)), "null out": groups(g=((p, 2, 3, None),)),
           "B": groups(g=((p, 0, 3, p),)), "T": groups(g=((p, 2, 0, p),)), "second group": groups(g=((p, 2, 3, p), (p, 2, -1, p)))}
    assert all(rc == -1 for rc in bad.values()), bad
    assert _lib.internal_noise_bits(None, 1, 1, 80, 0, 1, 0, p, s) == -1 and _lib.internal_noise_bits(p, 1, 1, 80, 0, 1, -1, p, s) == -1

    f = (C.c_float * 4)()
    assert lib.cmtts_sample_seeded_workspace_bytes(None, 1, 1, 1) == 0
    assert lib.cmtts_sample_seeded(None, p, p, None, 1, 1, 1, f, f, p, p, 1 << 20, s, None, None, 0, 0, None, None) == -1
    cfg = _lib.CMTTSConfigStruct()
    h = C.c_void_p()
    assert lib.cmtts_create(C.byref(cfg), C.byref(h)) == 0
    try:          # a model that is not finalized: rejected before anything else
        assert lib.cmtts_sample_seeded(h, p, p, None, 1, 1, 1, f, f, p, p, 1 << 20, s, None, None, 0, 0, None, None) == -1
    finally:
        lib.cmtts_destroy(h)
