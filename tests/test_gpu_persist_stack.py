"""The persistent denoiser stack called ALONE through its three exported launchers (cm-tts_amd/csrc/persist_args.h: cmtts_launch_denoiser_persist,
_persist_lp, _persist_ragged) against the float64 definition of the same operation (tests/persist_stack_cases.py: denoiser_kernel_cases.block_def
chained over the layers, then the skip head and the post-scaling) and, where an instance has a per-layer twin, bit for bit against NL chained
per-layer launches on the same buffers.  Until this module the stack was pinned only through whole 20 - 30 layer models, on the 80-channel mel
behind the skip head.

  A  fp32 direct (wino 0), tail off: the skip sum within M yard of float64 AND bit for bit NL chained cmtts_launch_resblock launches
  B  F(4,3) (wino 3): within M yard; bit for bit NL chained cmtts_launch_resblock_w43 launches at every residue of T (batch_invariant's promise)
  C  F(2,3) (wino 1): within M yard — it has no twin
  D  bf16, fp16 (lp modes 1, 2): bit for bit NL chained cmtts_launch_resblock_lp launches (the chain carries the float64 anchor of
     tests/test_gpu_denoiser_kernels.py; rounding flips over several layers make a direct bound meaningless); fp16x3 (mode 3): within M yard of
     float64 on operands rounded to hi + lo fp16, and not the fp32 direct result's bits
  E  the tail on (direct, F(4,3), bf16, fp16x3): out [B][T][80] within M yard of tail_def o stack_def — launch scalars with and without xold /
     noise, two post_rows tables (re-noised with nstd = 0; not re-noised with the noise pointer there; FINAL -> out_final, `out` keeps the
     sentinel there); `skip` keeps the sentinel.  bf16: the tail alone on the launch's own tail-off skip sum (D anchors that bit for bit)
  F  FACT (direct, F(4,3); tail on and off; cp = NULL): bit for bit the plain instance on DC.expand_def's cp, and within M yard
  G  chunks: B = 3 at max_blocks = tiles (1 + 1 + 1), 2 tiles (2 + 1), T = 129 at 2 tiles + 1 (remainder) bit for bit the single launch
  H  ragged: two groups (B = 2, T = 129; B = 1, T = 65), shuffled descriptors, untrimmed utterances bit for bit their group's uniform launch; one
     trimmed to active = 1: frames < 64 within M yard of the definition at T = 64, frames >= 64 keep the sentinel; the same with FACT
  I  utterance 1 alone; the launch behind one on inputs 1e4 x larger with the same halo / xst buffers; halo_zeroed = 1 on a halo the test cleared
  J  refusals: -2, nothing written — B = 0 and T = 0 with force (an integer division by zero before the guards that came with this module)

Every launch: force = 1, max_blocks <= the CU count (the residency rule the neighbour waits rest on), the cooperative switch untouched, `tmo` a
zeroed device word that must be 0 afterwards (nothing is retried), xst / halo handed over full of garbage, cp / dp / d with NL + 1 layers (the
last garbage), inputs between garbage rows and outputs between sentinel rows.  At the module's end cmtts_poll_error() == 0.

M = 10 (vocoder_kernel_cases.M), not set by what the kernels give; yard as in tests/persist_stack_cases.py.  That wrong kernels fail here is
shown on the CPU (tests/test_persist_stack_cases_cpu.py).  Measured worst ratios on MI355X: below the imports; every instance's is in the
report (PERSIST_F64 lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cmtts_amd  # noqa: F401
from cmtts_amd import _lib
from conftest import report
import denoiser_kernel_cases as DC
import persist_stack_cases as PC
import vocoder_kernel_cases as VC
import test_gpu_denoiser_kernels as DK
from test_gpu_denoiser_kernels import _between, _pack, _vec
from test_gpu_vocoder_kernels import _dev, _guard, _np, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
M = VC.M
CH, MEL, FN = PC.CH, PC.MEL, PC.FN
SENT = VC.SENTINEL
# Worst |kernel - float64| / yard per instance over its shapes, as measured on MI355X (256 CUs; the bound is M = 10 throughout; yard is 2e-6 .. 1e-5
# on a skip sum up to 4.8 and 5e-7 .. 5e-6 on an out up to 3).  No ratio above 1.6: nothing to explain.
#   skip sum, tail off: direct 1.02 (T = 129, NL = 2), F(4,3) 1.10 (T = 66) against the F(4,3) yardstick, F(2,3) 0.93, fp16x3 0.66 (yard = the 22-bit
#   operand model there); direct at 15, F(4,3) at 20, bf16 and fp16 at 15 shapes each bit for bit the per-layer chain
#   tail on: direct 1.54 (rows0, edge column), F(4,3) 1.19, fp16x3 0.99, bf16 1.25 (tail alone on its own skip sum)
#   FACT: bit for bit the plain instance on the expanded cp, tail off and on; direct 1.22, F(4,3) 1.13
#   chunks 1 + 1 + 1, 2 + 1, 2 + 1 with a remainder: bit for bit the single launch (direct; F(4,3) + FACT + post_rows + out_final; fp16x3 + tail)
#   ragged: both groups bit for bit their uniform launch; trimmed to active = 1: direct 0.78 / 0.71 (FACT), F(4,3) 0.69 / 0.55
#   alone, behind a 1e4 x larger launch on the same halo / xst, halo_zeroed = 1: same bits, all six instances; no tmo word set anywhere
#   refusals: the 32 excluded arguments all return -2 — B = 0, T = 0 and max_blocks < 1 in both uniform launchers and fact in the 16-bit one only
#   since the guards that came with this module

_VP, _I = C.c_void_p, C.c_int


def _clib():
    lib = DK._clib()
    lib.cmtts_launch_denoiser_persist.restype, lib.cmtts_launch_denoiser_persist.argtypes = _I, [_VP, _I, _I, _VP]
    lib.cmtts_launch_denoiser_persist_lp.restype, lib.cmtts_launch_denoiser_persist_lp.argtypes = _I, [_VP, _I, _I, _I, _VP]
    lib.cmtts_launch_denoiser_persist_ragged.restype, lib.cmtts_launch_denoiser_persist_ragged.argtypes = _I, [_VP, _VP]
    lib.cmtts_persist_state_floats.restype, lib.cmtts_persist_state_floats.argtypes = C.c_size_t, [_I, _I]
    lib.cmtts_persist_halo_bytes.restype, lib.cmtts_persist_halo_bytes.argtypes = C.c_size_t, [_I, _I]
    lib.cmtts_persist_chunks.restype, lib.cmtts_persist_chunks.argtypes = _I, [_I, _I, _I]
    lib.cmtts_persist_plan.restype, lib.cmtts_persist_plan.argtypes = _I, [_I, _I, _I, _I, _I]
    lib.cmtts_poll_error.restype, lib.cmtts_poll_error.argtypes = _I, []
    return lib


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module", autouse=True)
def _error_word():
    lib = _clib()
    torch.cuda.synchronize()
    lib.cmtts_poll_error()          # (what earlier modules left is theirs)
    yield
    torch.cuda.synchronize()
    assert lib.cmtts_poll_error() == 0, "the process-wide error word was set during this module"


class Worst(DK.Worst):
    def line(self, name):
        r, e, y, T, what = self.w
        assert self.n > 0, (name, "nothing was compared")
        report(f"PERSIST_F64 {name}: |d| {e:.2e}, yard {y:.2e}, ratio {r:.2f} at T={T} ({what}); edge and seam columns {self.seam:.2f}; largest |d| of all {self.raw:.2e}")
        return r


# ----------------------------------------------------------------------------------------------------------------- buffers and launches

_LAY3 = {"direct": "fragment_order", "f23": "wino_fragments", "f43": "wino43_fragments", "bf16": "fragment16", "fp16": "fragment16", "fp16x3": "fragment16_split"}
_LAYO = {"bf16": "fragment16", "fp16": "fragment16", "fp16x3": "fragment16_split"}
_PACK_MODE = {"bf16": 1, "fp16": 2}


def _weights(inst, NL):
    """Per layer (W3f, b3, Wof, bo) device pointers as import.hip packs them: rows of W3 and b3 in gate_perm(16) order."""
    lay3, layo, pm = _LAY3[inst], _LAYO.get(inst, "fragment_order"), _PACK_MODE.get(inst, 0)
    out = []
    for l in range(NL):
        W3, b3, Wo, bo = PC.layer_weights(l)
        out.append((_pack(("ps", l, "W3", lay3, pm), lay3, DC.permuted_kmajor(W3), pm), _vec(("ps", l, "b3"), lambda: b3[DC.gate_perm(16)]),
                    _pack(("ps", l, "Wo", layo, pm), layo, VC.kmajor(Wo[:, :, None]), pm), _vec(("ps", l, "bo"), lambda: bo)))
    return out


def _tail_weights():
    Ws, bs, Wp, bp = PC.tail_weights()
    Wp96 = np.zeros((96, CH), F32)
    Wp96[:MEL] = Wp
    return (_pack(("ps", "Ws"), "fragment_order", VC.kmajor(Ws[:, :, None])), _vec(("ps", "bs"), lambda: bs),
            _pack(("ps", "Wp"), "fragment_order", VC.kmajor(Wp96[:, :, None])), _vec(("ps", "bp"), lambda: bp))


_STALE = (1 << 32) | int(np.asarray(1e4, F32).view(np.uint32))      # a granule that looks published: layer tag 1, value 1e4


class State:
    """halo and xst of a (Bn, T) batch, each between two guard words, handed to the launch full of garbage (the launcher clears the halo unless
    halo_zeroed; xst is the Winograd instances' private state, written before it is read)."""

    def __init__(self, lib, Bn, T):
        self.nh = lib.cmtts_persist_halo_bytes(Bn, T) // 8
        self.nx = lib.cmtts_persist_state_floats(Bn, T)
        tiles = (T + FN - 1) // FN
        assert self.nh == 2 * Bn * tiles * 2 * CH and self.nx == Bn * tiles * 16384
        self.halo = torch.full((self.nh + 2,), _STALE, dtype=torch.int64, device=DEV)
        self.xst = torch.full((self.nx + 8,), float(PC.GARBAGE), device=DEV)      # (four guard floats either side: the state moves 16 bytes per lane)

    def clear_halo(self):
        self.halo[1:-1] = 0

    def check(self):
        assert int(self.halo[0]) == _STALE and int(self.halo[-1]) == _STALE, "written outside the halo granules"
        assert (self.xst[:4] == PC.GARBAGE).all() and (self.xst[-4:] == PC.GARBAGE).all(), "written outside xst"


class Bufs:
    """The device buffers of one (Bn, T) batch as a launch (or a ragged group) takes them."""

    def __init__(self, lib, NL, x0, cp, dp, d, fact=None, tailv=None, state=None):
        Bn, _, T = x0.shape
        self.Bn, self.T, self.NL, self.tailv = Bn, T, NL, tailv
        self.state = State(lib, Bn, T) if state is None else state
        self.x0 = _between(x0, PC.GARBAGE)
        self.cp = None if fact is not None else _between(PC.alloc_layers(cp, NL), PC.GARBAGE)
        self.dp, self.d = _dev(PC.alloc_layers(dp, NL)), _dev(PC.alloc_layers(d, NL))
        self.skip = _guard(Bn, CH, T)
        self.fact = None if fact is None else [_dev(v) for v in fact]      # p1, p2, p1t, p2t, mel2ph, pidx
        self.xold = self.noise = self.rows = self.out = self.outf = None
        self.table = False
        if tailv is not None:
            rows, wx, wn, self.table = PC.tail_post(tailv, Bn)
            xold, noise = PC.post_inputs(T, Bn)
            self.rows_np = rows
            self.xold = _between(xold, PC.GARBAGE) if wx else None
            self.noise = _between(noise, PC.GARBAGE) if wn else None
            self.out, self.outf = _guard(Bn, T, MEL), _guard(Bn, T, MEL)
            if self.table:      # PostRow [Bn] between two rows that would re-noise by 1e4 and send the rows to out_final
                tab = np.zeros(Bn + 2, np.dtype([("c_out", "f4"), ("c_skip", "f4"), ("nstd", "f4"), ("flags", "u4")]))
                tab[0] = tab[-1] = (1e4, 1e4, 1e4, 3)
                for b in range(Bn):
                    tab[b + 1] = (rows[b, 0], rows[b, 1], rows[b, 2], int(rows[b, 3]))
                assert tab.itemsize == C.sizeof(PC.PostRow)
                self.rows = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)

    def skip_rows(self, finite=True):
        return _rows(self.skip, self.T, finite)

    def skip_untouched(self):
        assert (_np(self.skip) == SENT).all(), "the tail form wrote the skip sum"

    def out_rows(self, only=None):
        """[Bn][T][80] from `out`, FINAL utterances from out_final; every other row of either buffer keeps the sentinel.  only: {b: frames} — the
        utterances that ran and how many frames of each (a ragged launch that left some out, or trimmed one)."""
        o, f = _np(self.out), _np(self.outf)
        for t in (o, f):
            assert (t[0] == SENT).all() and (t[-1] == SENT).all(), "written outside the launch's rows"
        got = np.full((self.Bn, self.T, MEL), np.nan, F32)
        for b in range(self.Bn):
            final = self.table and int(self.rows_np[b, 3]) & PC.POSTROW_FINAL
            n = self.T if only is None else only.get(b, 0)
            src, other = (f, o) if final else (o, f)
            assert (other[b + 1] == SENT).all(), (b, "FINAL" if final else "not FINAL", "the other destination was written")
            assert (src[b + 1, n:] == SENT).all(), (b, "written beyond the utterance's frames")
            got[b, :n] = src[b + 1, :n]
            assert np.isfinite(got[b, :n]).all()
        return got


def _model_args(a, inst, NL, tail):
    for l, (w3, b3, wo, bo) in enumerate(_weights(inst, NL)):
        a.W3f[l], a.b3[l], a.Wof[l], a.bo[l] = w3, b3, wo, bo
    a.NL, a.vec_stride, a.wino = NL, (NL + 1) * CH, PC.WINO.get(inst, 0)
    if tail:
        a.tail, a.n_mels, a.skip_div = 1, MEL, float(F32(np.sqrt(float(NL))))
        a.Wsf, a.bs, a.Wpf, a.bp = _tail_weights()
        a.c_out, a.c_skip, a.nstd = PC.POST_SCALARS


def _ptr(t, row=1):
    return None if t is None else t[row:].data_ptr()


def _fact_args(a, g, bf, NL):
    p1, p2, p1t, p2t, m2p, pix = bf.fact
    a.fact, a.p2, a.p2t, a.ld2 = 1, p2.data_ptr(), p2t.data_ptr(), PC.EXPAND_LD2
    g.p1, g.p1t, g.mel2ph, g.pidx, g.ldp, g.Lph = p1.data_ptr(), p1t.data_ptr(), m2p.data_ptr(), pix.data_ptr(), PC.EXPAND_LDP, PC.EXPAND_L


def _launch(lib, inst, bf, max_blocks=None, halo_zeroed=0, tmo_ok=(0,), what=""):
    """One call of the uniform launcher of `inst` on bf's buffers (force = 1) -> nothing; the results are read from bf."""
    NL, Bn, T = bf.NL, bf.Bn, bf.T
    a = PC.PersistArgs()
    _model_args(a, inst, NL, bf.tailv is not None)
    a.x0, a.cp, a.dp, a.d, a.skip = _ptr(bf.x0), _ptr(bf.cp), bf.dp.data_ptr(), bf.d.data_ptr(), _ptr(bf.skip)
    a.cp_bstride, a.B, a.T = (NL + 1) * CH * T, Bn, T
    a.halo, a.halo_zeroed = _ptr(bf.state.halo), halo_zeroed
    a.xst = _ptr(bf.state.xst, 4) if inst in PC.WINO else None
    if bf.fact is not None:
        _fact_args(a, a, bf, NL)
    if bf.tailv is not None:
        a.xold, a.noise, a.out = _ptr(bf.xold), _ptr(bf.noise), _ptr(bf.out)
        if bf.table:
            a.c_out = a.c_skip = a.nstd = 1e3          # the table decides, not the launch scalars
            a.post_rows, a.out_final = bf.rows.data_ptr() + C.sizeof(PC.PostRow), _ptr(bf.outf)
    tmo = torch.zeros(2, dtype=torch.int32, device=DEV)
    a.tmo = tmo.data_ptr()
    cus = _cus()
    mb = cus if max_blocks is None else max_blocks
    assert 1 <= mb <= cus
    if inst in PC.LP_MODE:
        rc = lib.cmtts_launch_denoiser_persist_lp(C.byref(a), PC.LP_MODE[inst], mb, 1, None)
    else:
        rc = lib.cmtts_launch_denoiser_persist(C.byref(a), mb, 1, None)
    torch.cuda.synchronize()
    assert rc == 0, (inst, NL, Bn, T, what, rc)
    word = _np(tmo).tolist()
    assert word[0] in tmo_ok and word[1] == 0, f"tmo word {word} after {inst} NL={NL} B={Bn} T={T} max_blocks={mb} {what}"
    bf.state.check()


def _run(lib, inst, NL, T, Bn=PC.B, fact=False, tailv=None, max_blocks=None, xs=None, state=None, halo_zeroed=0, finite=True, tmo_ok=(0,)):
    """A uniform launch on the case (T, Bn) — or on xs = (x0, cp, dp, d) — -> the skip sum [Bn][C][T] (tail off) or out [Bn][T][80]."""
    x0, cp, dp, d = PC.case_inputs(T, Bn, fact) if xs is None else xs
    bf = Bufs(lib, NL, x0, cp, dp, d, PC.fact_tables(T, Bn, NL) if fact else None, tailv, state)
    _launch(lib, inst, bf, max_blocks, halo_zeroed, tmo_ok)
    if tailv is None:
        return bf.skip_rows(finite)
    bf.skip_untouched()
    return bf.out_rows()


_PER_LAYER = {"direct": "cmtts_launch_resblock", "f43": "cmtts_launch_resblock_w43", "bf16": "cmtts_launch_resblock_lp", "fp16": "cmtts_launch_resblock_lp"}


def _chain(lib, inst, NL, T, Bn=PC.B):
    """NL chained per-layer launches (accum_skip from layer 1) on the same allocation -> the skip sum [Bn][C][T]."""
    x0, cp, dp, d = PC.case_inputs(T, Bn)
    bf = Bufs(lib, NL, x0, cp, dp, d)
    xs = [bf.x0] + [_guard(Bn, CH, T) for _ in range(NL)]
    z = _guard(Bn, CH, T)
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    fn = getattr(lib, _PER_LAYER[inst])
    for l, (w3, b3, wo, bo) in enumerate(_weights(inst, NL)):
        a = DC.ResArgs(x_in=_ptr(xs[l]), cp=_ptr(bf.cp) + 4 * l * CH * T, dp=bf.dp.data_ptr() + 4 * l * CH, d=bf.d.data_ptr() + 4 * l * CH, x_out=_ptr(xs[l + 1]),
                       skip=_ptr(bf.skip), W3f=w3, b3=b3, Wof=wo, bo=bo, cp_bstride=(NL + 1) * CH * T, vec_stride=(NL + 1) * CH, B=Bn, T=T, accum_skip=int(l > 0),
                       z=_ptr(z), flag=flag.data_ptr())
        rc = fn(C.byref(a), PC.LP_MODE[inst], None) if inst in PC.LP_MODE else fn(C.byref(a), None)
        assert rc == 0, (inst, l, T, rc)
    torch.cuda.synchronize()
    assert int(flag[0]) == 0, (inst, T, "the per-layer overflow word")
    return bf.skip_rows()


_SKIP = {}


def _skip_of(lib, inst, NL, T):
    """The tail-off skip sum of (inst, NL, T) at B = PC.B: launched once per module."""
    key = (inst, NL, T)
    if key not in _SKIP:
        _SKIP[key] = _run(lib, inst, NL, T)
    return _SKIP[key]


def _vs_f64(lib, inst, twin, NLs=PC.NLS):
    worst = Worst(FN)
    n = 0
    for NL in NLs:
        for T in PC.t_list(inst, NL):
            got = _skip_of(lib, inst, NL, T)
            ref, yard = PC.stack_reference(inst, NL, T)
            worst.add(got - ref, yard, T, f"skip NL={NL}")
            if twin:
                assert np.array_equal(got, _chain(lib, inst, NL, T)), (inst, NL, T, "differs from the chained per-layer launches")
                n += 1
    r = worst.line(f"{inst} skip sum, tail off" + (f"; {n} shapes bit for bit the per-layer chain" if twin else ""))
    assert r <= M, (inst, worst.w)


# ----------------------------------------------------------------------------------------------------------------- A - D: the skip sum

def test_direct_vs_f64_and_per_layer_chain():
    """A: denoiser_persist_kernel<.., WINO = 0>, tail off, NL in {1, 2, 3}: the skip sum within M yard of stack_def in float64 and bit for bit NL
    chained resblock_fused launches; rows and columns of `skip` outside the launch keep the sentinel (_rows)."""
    _vs_f64(_clib(), "direct", True)


def test_f43_vs_f64_and_per_layer_chain():
    """B: the F(4,3) instance (wino = 3) against float64 with the F(4,3) restatement's float32 yardstick, and bit for bit NL chained
    cmtts_launch_resblock_w43 launches at every residue of T mod 4 — what the batch_invariant option promises."""
    _vs_f64(_clib(), "f43", True)


def test_f23_vs_f64():
    """C: the F(2,3) instance (wino = 1) exists as the persistent stack only: float64 with the F(2,3) restatement's yardstick is its one anchor."""
    _vs_f64(_clib(), "f23", False)


@pytest.mark.parametrize("inst", ["bf16", "fp16"])
def test_lp_is_the_per_layer_chain(inst):
    """D: bf16 / fp16 stacks bit for bit NL chained resblock_fused_lp launches at the full T list (that kernel is anchored in float64 by
    tests/test_gpu_denoiser_kernels.py); the fp16 overflow word (code 3 in tmo) stays clear; the result is not the fp32 stack's."""
    lib = _clib()
    n = 0
    for NL, T in PC.shapes(inst):
        got = _skip_of(lib, inst, NL, T)
        assert np.array_equal(got, _chain(lib, inst, NL, T)), (inst, NL, T, "differs from the chained per-layer launches")
        ref, yard = PC.stack_reference("direct", NL, T)
        assert np.abs(got - _skip_of(lib, "direct", NL, T)).max() > 50 * yard, (inst, NL, T, "the 16-bit launch gave the fp32 kernel's result")
        n += 1
    report(f"PERSIST_F64 {inst} skip sum, tail off: {n} shapes bit for bit the per-layer chain")


def test_fp16x3_vs_f64():
    """D: fp16x3 (lp mode 3) exists as the persistent stack only: within M yard of float64 on operands rounded to hi + lo fp16 (yard floored by the
    22-bit operand model), no rounding-flip widening; not the bits of the fp32 direct stack."""
    lib = _clib()
    _vs_f64(lib, "fp16x3", False)
    for T in (65, 129):
        assert not np.array_equal(_skip_of(lib, "fp16x3", 3, T), _skip_of(lib, "direct", 3, T)), (T, "fp16x3 gave the fp32 stack's bits")


# ----------------------------------------------------------------------------------------------------------------- E: the tail

TAIL_SHAPES = [(3, T, v) for T in (1, 64, 65, 129) for v in PC.TAIL_VARIANTS] + [(NL, 65, v) for NL in (1, 2) for v in ("full", "rows0")]


@pytest.mark.parametrize("inst", ["direct", "f43", "bf16", "fp16x3"])
def test_tail_vs_f64(inst):
    """E: persist_tail.h inside the launch: out within M yard of tail_def o stack_def (yard from the float32 evaluation of the whole composition); bf16:
    of tail_def on the launch's own tail-off skip sum.  _run checks that `skip` keeps the sentinel, Bufs.out_rows that FINAL rows are in out_final
    with `out` untouched there (and the other way round), and that the launch scalars are not used when a table is given."""
    lib = _clib()
    worst = Worst(FN)
    for NL, T, v in TAIL_SHAPES:
        got = _run(lib, inst, NL, T, tailv=v)
        if inst == "bf16":
            ref, yard = PC.tail_on_skip_reference(_skip_of(lib, inst, NL, T), NL, T, v)
        else:
            ref, yard = PC.tail_reference(inst, NL, T, v)
        worst.add(np.transpose(got - ref, (0, 2, 1)), yard, T, f"out NL={NL} {v}")
    assert worst.line(f"{inst} tail on, out") <= M, (inst, worst.w)


# ----------------------------------------------------------------------------------------------------------------- F: FACT

@pytest.mark.parametrize("inst", ["direct", "f43"])
def test_fact_is_the_expanded_cp(inst):
    """F: the FACT instances (cp = NULL, the conditioner projections gathered from p1 / p2 / p1t / p2t with mel2ph holding padding frames and values
    above Lph, pidx values outside the table) bit for bit the plain instance on DC.expand_def's cp, tail off and on, and within M yard of float64.
    NL = 2 as well: utterance 1's factors start NL C ldp floats in."""
    lib = _clib()
    worst = Worst(FN)
    for NL, T in [(3, T) for T in (1, 64, 65, 129)] + [(2, 65), (1, 129)]:
        xs = PC.case_inputs(T, PC.B, True)
        got = _run(lib, inst, NL, T, fact=True)
        assert np.array_equal(got, _run(lib, inst, NL, T, xs=xs)), (inst, NL, T, "FACT differs from the plain instance on the expanded cp")
        ref, yard = PC.stack_reference(inst, NL, T, PC.B, True)
        worst.add(got - ref, yard, T, f"skip NL={NL}")
        for v in ("full", "rows0"):
            out = _run(lib, inst, NL, T, fact=True, tailv=v)
            assert np.array_equal(out, _run(lib, inst, NL, T, xs=xs, tailv=v)), (inst, NL, T, v, "FACT + tail differs from the plain instance")
            ref, yard = PC.tail_reference(inst, NL, T, v, PC.B, True)
            worst.add(np.transpose(out - ref, (0, 2, 1)), yard, T, f"out NL={NL} {v}")
    assert worst.line(f"{inst} FACT, tail off and on") <= M, (inst, worst.w)


# ----------------------------------------------------------------------------------------------------------------- G: chunks

@pytest.mark.parametrize("inst,fact,tailv", [("direct", False, None), ("f43", True, "rows1"), ("fp16x3", False, "full")])
def test_chunks_are_the_single_launch(inst, fact, tailv):
    """G: the launchers' balanced utterance chunks (pointer offsets of halo — the parity stride keeps a.B —, xst, post_rows + b0, out_final, the
    factor tables), reached at B = 3 by lowering max_blocks: 1 + 1 + 1 and 2 + 1 utterances at T = 65, 2 + 1 at T = 129 with a remainder; each
    bit for bit the single launch at the CU count.  cmtts_persist_chunks answers the same counts."""
    lib = _clib()
    NL, Bn = 3, 3
    for T, blocks in ((65, (2, 4)), (129, (7,))):
        tiles = (T + FN - 1) // FN
        assert lib.cmtts_persist_chunks(Bn, T, _cus()) == 1
        one = _run(lib, inst, NL, T, Bn, fact, tailv)
        for mb in blocks:
            want = PC.chunks_expected(Bn, T, mb)
            assert len(want) > 1 and lib.cmtts_persist_chunks(Bn, T, mb) == len(want), (T, mb, want)
            assert lib.cmtts_persist_plan(Bn, T, NL, mb, 1) == tiles * want[0]
            got = _run(lib, inst, NL, T, Bn, fact, tailv, max_blocks=mb)
            assert np.array_equal(got, one), (inst, T, mb, want, "the chunked call differs from the single launch")
    report(f"PERSIST_F64 {inst} chunks (fact={int(fact)}, tail={tailv}): 1+1+1, 2+1 and 2+1 with a remainder bit for bit the single launch")


# ----------------------------------------------------------------------------------------------------------------- H: ragged

def _ragged(lib, inst, NL, groups, trims, fact, order):
    """One ragged launch, tail on with the launch scalars ("full").  groups: [(T, Bn)]; trims: {(g, b): active tiles}; -> per group out [Bn][T][80]
    (frames a trimmed utterance did not compute: NaN)."""
    a = PC.PersistArgs()
    _model_args(a, inst, NL, True)
    a.halo_zeroed, a.n_groups = 1, len(groups)
    bfs, descs = [], []
    for g, (T, Bn) in enumerate(groups):
        x0, cp, dp, d = PC.case_inputs(T, Bn, fact)
        bf = Bufs(lib, NL, x0, cp, dp, d, PC.fact_tables(T, Bn, NL) if fact else None, "full")
        bf.state.clear_halo()          # the ragged launcher leaves that to its caller
        pg = a.grp[g]
        pg.x0, pg.cp, pg.dp, pg.d, pg.skip = _ptr(bf.x0), _ptr(bf.cp), bf.dp.data_ptr(), bf.d.data_ptr(), _ptr(bf.skip)
        pg.halo, pg.xst = _ptr(bf.state.halo), _ptr(bf.state.xst, 4)
        pg.xold, pg.noise, pg.out = _ptr(bf.xold), _ptr(bf.noise), _ptr(bf.out)
        pg.cp_bstride, pg.B, pg.T, pg.tiles = (NL + 1) * CH * T, Bn, T, (T + FN - 1) // FN
        if fact:
            _fact_args(a, pg, bf, NL)
        for b in range(Bn):
            act = trims.get((g, b), pg.tiles)
            descs += [PC.desc_word(g, b, t, act) for t in range(act)]
        bfs.append(bf)
    descs = [descs[i] for i in order(len(descs))]
    assert len(descs) <= _cus()
    a.n_wg = len(descs)
    for i, w in enumerate(descs):
        a.desc[i] = w
    tmo = torch.zeros(2, dtype=torch.int32, device=DEV)
    a.tmo = tmo.data_ptr()
    rc = lib.cmtts_launch_denoiser_persist_ragged(C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, (inst, fact, rc)
    assert _np(tmo).tolist() == [0, 0], f"tmo word {_np(tmo).tolist()} after ragged {inst} fact={fact} trims={trims}"
    outs = []
    for g, bf in enumerate(bfs):
        bf.state.check()
        bf.skip_untouched()
        outs.append(bf.out_rows({b: min(bf.T, trims.get((g, b), 99) * FN) for b in range(bf.Bn)}))
    return outs


@pytest.mark.parametrize("fact", [False, True])
@pytest.mark.parametrize("inst", ["direct", "f43"])
def test_ragged_groups_and_trim(inst, fact):
    """H: the ragged launcher's descriptor decoding: two groups with their own T and buffers in one launch, the descriptor list shuffled (a
    workgroup's place in the grid means nothing), halos cleared by the test.  Untrimmed utterances bit for bit their group's uniform launch;
    utterance 1 of group 0 trimmed to one active tile: frames < 64 within M yard of the definition at T = 64 — the frames beyond behave like
    frames beyond T —, frames >= 64 keep the sentinel, and the other utterances keep their bits."""
    lib = _clib()
    NL, groups = 3, [(129, 2), (65, 1)]
    uniform = [_run(lib, inst, NL, T, Bn, fact, "full") for T, Bn in groups]
    shuffled = lambda n: np.random.RandomState(77).permutation(n)
    outs = _ragged(lib, inst, NL, groups, {}, fact, shuffled)
    for g in range(2):
        assert np.array_equal(outs[g], uniform[g]), (inst, fact, g, "a ragged group differs from its uniform launch")
    outs = _ragged(lib, inst, NL, groups, {(0, 1): 1}, fact, shuffled)
    assert np.array_equal(outs[0][0], uniform[0][0]) and np.array_equal(outs[1], uniform[1]), (inst, fact, "a neighbour's trim moved an untrimmed utterance")
    ref, yard = PC.tail_reference(inst, NL, 129, "full", PC.B, fact, FN)
    worst = Worst(FN)
    worst.add(np.transpose(outs[0][1, :FN] - ref[1], (1, 0))[None], yard, FN, "out of the trimmed utterance")
    assert np.abs(outs[0][1, :FN - NL] - uniform[0][1, :FN - NL]).max() <= M * yard      # and far from the cut it is the untrimmed result
    assert worst.line(f"{inst} ragged, fact={int(fact)}: trimmed to active=1") <= M, worst.w


# ----------------------------------------------------------------------------------------------------------------- I: alone and stale

@pytest.mark.parametrize("inst", PC.INSTANCES)
def test_alone_and_stale(inst):
    """I: utterance 1 launched alone has its bits from the batch; the launch repeated behind one on inputs 1e4 x larger, on the SAME halo and xst
    buffers which the test does not clear in between, has the same bits (the launcher's clearing, xst written before it is read); and again with
    halo_zeroed = 1 on a halo the test cleared.  (The 1e4 x launch leaves the fp16 range: code 3 in ITS tmo word is the fp16 modes' answer.)"""
    lib = _clib()
    NL = 3
    for T in (1, 65):
        x0, cp, dp, d = PC.case_inputs(T)
        got = _skip_of(lib, inst, NL, T)
        one = _run(lib, inst, NL, T, 1, xs=(x0[1:2], cp[1:2], dp[1:2], d[1:2]))
        assert np.array_equal(one[0], got[1]), (inst, T, "utterance 1 alone differs from its rows in the batch")
        st = State(lib, PC.B, T)
        big = F32(1e4)
        _run(lib, inst, NL, T, xs=(x0 * big, cp * big, dp * big, d * big), state=st, finite=False, tmo_ok=(0, 3) if inst in ("fp16", "fp16x3") else (0,))
        assert np.array_equal(_run(lib, inst, NL, T, state=st), got), (inst, T, "the launch depends on what ran before it")
        st.clear_halo()
        assert np.array_equal(_run(lib, inst, NL, T, state=st, halo_zeroed=1), got), (inst, T, "halo_zeroed = 1 on a cleared halo changes the bits")


# ----------------------------------------------------------------------------------------------------------------- J: refusals

def test_refusals():
    """J: what the launchers' header excludes returns -2 and writes nothing.  Every call carries complete, valid buffers of a (B = 2, T = 65, NL = 2)
    batch, so a launcher that wrongly accepted would run in bounds and fail the sentinel check.  B = 0 and T = 0 with force were an integer
    division by zero in both uniform launchers until the guards that came with this module (read from the code, never run)."""
    lib = _clib()
    NL, T, Bn = 2, 65, PC.B
    cus = _cus()
    x0, cp, dp, d = PC.case_inputs(T, Bn)
    bf = Bufs(lib, NL, x0, cp, dp, d, None, "rows0")
    bf.cp_keep = bf.cp
    ft = [_dev(v) for v in PC.fact_tables(T, Bn, NL)]
    tmo = torch.zeros(2, dtype=torch.int32, device=DEV)

    def args(inst, tail=False, **kw):
        a = PC.PersistArgs()
        _model_args(a, inst, NL, tail)
        a.x0, a.cp, a.dp, a.d, a.skip = _ptr(bf.x0), _ptr(bf.cp), bf.dp.data_ptr(), bf.d.data_ptr(), _ptr(bf.skip)
        a.cp_bstride, a.B, a.T, a.halo, a.xst, a.tmo = (NL + 1) * CH * T, Bn, T, _ptr(bf.state.halo), _ptr(bf.state.xst, 4), tmo.data_ptr()
        a.xold, a.noise, a.out, a.out_final, a.post_rows = _ptr(bf.xold), _ptr(bf.noise), _ptr(bf.out), _ptr(bf.outf), bf.rows.data_ptr() + 16
        a.p1, a.p2, a.p1t, a.p2t, a.mel2ph, a.pidx = (t.data_ptr() for t in (ft[0], ft[1], ft[2], ft[3], ft[4], ft[5]))
        a.ldp, a.Lph, a.ld2 = PC.EXPAND_LDP, PC.EXPAND_L, PC.EXPAND_LD2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    fp32 = lambda a, mb=cus: lib.cmtts_launch_denoiser_persist(C.byref(a), mb, 1, None)
    lp = lambda a, mode=1, mb=cus: lib.cmtts_launch_denoiser_persist_lp(C.byref(a), mode, mb, 1, None)
    rcs = {}
    for name, fn, inst in (("persist", fp32, "direct"), ("persist_lp", lp, "bf16")):
        rcs[name + " B=0"] = fn(args(inst, B=0))
        rcs[name + " T=0"] = fn(args(inst, T=0))
        rcs[name + " B=0 T=0 tail"] = fn(args(inst, True, B=0, T=0))
        rcs[name + " NL=0"] = fn(args(inst, NL=0))
        rcs[name + " NL=33"] = fn(args(inst, NL=33))
        rcs[name + " tiles > max_blocks"] = fn(args(inst), mb=1)
        rcs[name + " max_blocks=0"] = fn(args(inst), mb=0)
        rcs[name + " max_blocks=-1"] = fn(args(inst), mb=-1)
    rcs["persist wino=2"] = fp32(args("direct", wino=2))
    rcs["persist wino=1 xst=null"] = fp32(args("f23", xst=None))
    rcs["persist wino=3 xst=null"] = fp32(args("f43", xst=None))
    for miss in ("p1t", "p2t", "mel2ph"):
        rcs[f"persist fact {miss}=null"] = fp32(args("direct", fact=1, cp=None, **{miss: None}))
    rcs["persist_lp mode=0"] = lp(args("bf16"), mode=0)
    rcs["persist_lp mode=4"] = lp(args("bf16"), mode=4)
    rcs["persist_lp fact=1"] = lp(args("bf16", fact=1))
    assert lib.cmtts_persist_chunks(0, T, cus) == 0 and lib.cmtts_persist_chunks(Bn, 0, cus) == 0 and lib.cmtts_persist_chunks(Bn, T, 0) == 0
    assert lib.cmtts_persist_plan(Bn, 0, NL, cus, 1) == 0 and lib.cmtts_persist_plan(0, T, NL, cus, 1) == 0 and lib.cmtts_persist_plan(Bn, T, NL, 0, 1) == 0

    def ragged(n_wg=2, n_groups=1, tiles=2, **kw):
        a = args("direct", True, halo_zeroed=1, n_groups=n_groups, n_wg=n_wg, **kw)
        for g in range(PC.MAX_GROUPS):
            pg = a.grp[g]
            pg.x0, pg.cp, pg.dp, pg.d, pg.skip, pg.halo, pg.xst = a.x0, a.cp, a.dp, a.d, a.skip, a.halo, a.xst
            pg.xold, pg.noise, pg.out, pg.cp_bstride, pg.B, pg.T, pg.tiles = a.xold, a.noise, a.out, a.cp_bstride, 1, T, tiles
        a.desc[0], a.desc[1] = PC.desc_word(0, 0, 0, 2), PC.desc_word(0, 0, 1, 2)
        return lib.cmtts_launch_denoiser_persist_ragged(C.byref(a), None)

    rcs["ragged n_wg=0"] = ragged(n_wg=0)
    rcs["ragged n_wg=257"] = ragged(n_wg=257)
    rcs["ragged n_groups=9"] = ragged(n_groups=9)
    rcs["ragged n_groups=0"] = ragged(n_groups=0)
    rcs["ragged tiles=128"] = ragged(tiles=128)
    rcs["ragged NL=0"] = ragged(NL=0)
    rcs["ragged wino=2"] = ragged(wino=2)
    torch.cuda.synchronize()
    assert all(rc == -2 for rc in rcs.values()), {n: rc for n, rc in rcs.items() if rc != -2}
    for t in (bf.skip, bf.out, bf.outf):
        assert (_np(t) == SENT).all(), "a refused launch wrote"
    assert _np(tmo).tolist() == [0, 0]
    assert (_np(bf.state.halo) == _STALE).all(), "a refused launch touched the halo"
    report(f"PERSIST_F64 refusals: {len(rcs)} excluded arguments over the three launchers all returned -2")
