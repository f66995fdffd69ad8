#!/usr/bin/env python3
"""bench.py — mel-frames/s of the CM-TTS inference hot path on MI355X.

One "step" = one pass of the whole text->mel hot path over one synthetic batch per GPU:
FFT-block encoder -> variance adaptor / length regulator -> T=4 consistency sampling
(BASELINE.json configs[1]: LJSpeech model, batch 32, 80x512 mels, T=4, fp32), inputs resident in HBM,
the sampler's noise drawn on the device inside the step (as the reference draws it inside its sampler).  N>1: one process per GPU (launched by torch.distributed.run), every rank
runs its own batch (weak scaling, utterances shard with no data-path collective) and the step ends
with the single RCCL all-gather that collates the mels.

Prints ONE JSON line on rank 0 carrying, besides the headline value, `roofline` (dominant kernel: gated
k=3 Conv1D of the denoiser block, timed live with HIP events on its launch stream inside the timed steps).

A plain run does only what the headline needs: set up, warm up, time the steps, write --dump-outputs, print the
line.  `--full` adds everything that takes runs of its own: `extras` (other sampler step counts, precisions,
sizes and BASELINE configs, end-to-end wav, the vocoder alone; the N-GPU configs[3] / [4] blocks), `roofline_16bit`
and `cpu_baseline` (the numpy oracle timed on the host cores).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# CPU-baseline hygiene: OpenMP worker i stays on core i for the whole run (set before torch creates
# its thread pool), so the host-side timing does not depend on where the scheduler happens to move the workers
# — single-process runs only: under torch.distributed.run every rank would bind its initial thread to the same first core.
# Set with or without --full: the binding also places the thread that issues the timed steps, which must not move between the two.
if os.environ.get("WORLD_SIZE", "1") == "1":
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")

try:      # before torch starts OpenMP: with OMP_PROC_BIND the initial thread is bound to ONE core afterwards and the process's own mask is gone
    CPUS_AT_START = sorted(os.sched_getaffinity(0))
except AttributeError:
    CPUS_AT_START = list(range(os.cpu_count() or 1))

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import cmtts_amd  # noqa: E402
from cmtts_amd import _lib, host, shard  # noqa: E402
from cmtts_amd.config import get_config, HifiGanConfig  # noqa: E402
from cmtts_amd.weights import synth_cmtts_state_dict, synth_hifigan_state_dict  # noqa: E402

BATCH, PHONEMES, FRAMES_PAD, DUR = 32, 85, 512, 6      # 85 phonemes x 6 frames = 510 valid of 512 padded
N_STEPS = 4
FP32_MFMA_PEAK_TFLOPS = 157.3                           # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 peak
HBM_PEAK_GBS = 8000.0
DEVICE_SEED = 4321                                      # the device generator the in-step noise is drawn from (+ rank)
DUMP_LIMIT_BYTES = 64 << 20                             # --dump-outputs writes at most this much


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def make_inputs(cfg, seed, device):
    rs = np.random.RandomState(seed)
    texts = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(BATCH, PHONEMES)).astype(np.int64)).to(device)
    lens = torch.full((BATCH,), PHONEMES, dtype=torch.int64, device=device)
    gen = torch.Generator(device="cpu").manual_seed(1234 + seed)
    noise = torch.randn(N_STEPS + 1, BATCH, 1, FRAMES_PAD, cfg.n_mels, generator=gen).to(device)
    return texts, lens, noise


# HIP events bracket every 7th launch of the dominant kernel inside the timed region (7 is coprime to the 20
# layers, so all layers are sampled); bracketing every launch costs ~4 % of the step in event records.
PROFILE_STRIDE = 7


REDUCE_DEVICE = "cuda"      # where the max-over-ranks of a timed region is reduced (the CPU rehearsal of tests/test_shard_gloo.py sets "cpu")


def timed(fn, steps, warmup, world, before=None, flush=None):
    """`flush` completes whatever the last fn() left in flight (the async all-gather): it runs INSIDE the timed
    region, before the closing synchronize + barrier, so all K steps' work is counted."""
    for _ in range(warmup):
        fn()
    if flush is not None:
        flush()
    if before is not None:
        torch.cuda.synchronize()
        before()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    if flush is not None:
        flush()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=REDUCE_DEVICE)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    return dt


def vocoder_issued_flops_per_frame(winograd):
    """MFMA FLOPs the fp32 HiFi-GAN generator issues per mel frame (universal config: upsample 8, 8, 2, 2 from 512 channels; ResBlock kernels 3 / 7 / 11 x
    dilations 1 / 3 / 5), following the launcher's dispatch (cmtts_api.hip: cmtts_vocoder_forward) at its default switches for a launch of
    >= 1024 column tiles: products per output of a k-tap conv — direct k; F(4,3) tap groups (conv_xlq.hip) 6 / 16 / 24 per quad = 1.5 / 4 / 6; F(2,3) tap
    groups (conv_xlw) 4 / 10 / 15 per pair = 2 / 5 / 7.5.  A ResBlock = conv1 at dilation 1 / 3 / 5, each followed by a dilation-1 conv2.  (The fused pair
    kernels of the narrow stages recompute conv2's halo as well — 1-8 % of conv1, resblock_pair.hip — which this count has never included.)"""
    F43 = {3: 1.5, 7: 4.0, 11: 6.0}
    F23 = {3: 2.0, 7: 5.0, 11: 7.5}
    forms = {"direct": 0, "F(4,3)": 0, "F(2,3)": 0}
    total = 0.0
    rate = 1
    for C_, up in ((256, 8), (128, 8), (64, 2), (32, 2)):
        rate *= up
        for k in (3, 7, 11):
            for ci, dil in enumerate((1, 1, 3, 1, 5, 1)):          # conv1 d = 1, conv2, conv1 d = 3, conv2, conv1 d = 5, conv2
                if not winograd or C_ == 32:
                    per, form = float(k), "direct"
                elif k == 3 and C_ in (64, 128):
                    # round 6: the k = 3 pair in ONE launch (conv_xlq_pair.hip): conv1 recomputes conv2's halo — 64 xt frames per 60 outputs
                    # at dilation 1, 60 per 56 at dilation 3 / 5
                    per, form = F43[k] * ((64.0 / 60.0 if dil == 1 else 60.0 / 56.0) if ci % 2 == 0 else 1.0), "F(4,3)"
                elif dil in (1, 3) or C_ == 256 or k == 3:
                    per, form = F43[k], "F(4,3)"
                else:
                    per, form = F23[k], "F(2,3)"
                forms[form] += 1
                total += 2.0 * C_ * C_ * per * rate
    # conv_pre (80 -> 512, k = 7), the four ConvTranspose1d upsamplers (kernel 2 s: 2 s taps per input frame), conv_post (32 -> 1, k = 7): direct
    total += 2.0 * 80 * 512 * 7 + 2.0 * 512 * 256 * 16 + 2.0 * 256 * 128 * 16 * 8 + 2.0 * 128 * 64 * 4 * 64 + 2.0 * 64 * 32 * 4 * 128 + 2.0 * 32 * 7 * 256
    return {"flops_per_frame": total, "forms": forms}


def cpu_baseline(cfg, sd):
    """The numpy oracle (oracle/cmtts_oracle.py, pinned to the reference's golden vectors) timed on
    this box's host cores on a bounded sample of the same workload."""
    from oracle import cmtts_oracle as O
    O.set_backend("torch")            # oneDNN/MKL conv + GEMM primitives: what the reference's CPU path runs
    threads = torch.get_num_threads()
    all_threads = threads
    rs = np.random.RandomState(0)
    O.synthesize(sd, cfg, rs.randint(1, cfg.n_symbols, size=(1, 8)).astype(np.int64), np.asarray([8]), None, 1,
                 [rs.standard_normal(size=(1, 1, 48, cfg.n_mels)).astype(np.float32)])      # warm BLAS threads
    # the GPU step's own workload (full batch).  torch-CPU scaling on a 128-/256-thread host is not monotonic for tensors this
    # small, so the thread count is chosen ON THE TIMED BATCH SIZE: one pass per candidate, the scan reported;
    # then four more passes at the best count: `value` = best of its five, `median_value` = their median
    Bf = BATCH
    texts_f = rs.randint(1, cfg.n_symbols, size=(Bf, PHONEMES)).astype(np.int64)
    lens_f = np.full((Bf,), PHONEMES, np.int64)
    noise_f = [rs.standard_normal(size=(Bf, 1, FRAMES_PAD, cfg.n_mels)).astype(np.float32) for _ in range(N_STEPS + 1)]

    def one_pass():
        t0 = time.perf_counter()
        mel, mel_len, _ = O.synthesize(sd, cfg, texts_f, lens_f, None, N_STEPS, noise_f, max_mel_len=FRAMES_PAD, torch_sampler=True)
        return time.perf_counter() - t0, mel_len
    cands = sorted({min(all_threads, n) for n in (8, 16, 32, 64, 128, all_threads)})
    scan = {}
    for nt in cands:
        torch.set_num_threads(nt)
        scan[nt], mel_len = one_pass()
    best_threads = min(scan, key=scan.get)
    torch.set_num_threads(best_threads)
    runs = [scan[best_threads]]
    for _ in range(4):
        d, mel_len = one_pass()
        runs.append(d)
    torch.set_num_threads(all_threads)
    dt, med = min(runs), float(np.median(runs))
    O.set_backend("numpy")
    return {"value": round(float(mel_len.sum()) / dt, 1), "unit": "mel-frames/s", "cores": int(best_threads),
            "median_value": round(float(mel_len.sum()) / med, 1), "runs_s": [round(r, 3) for r in runs],
            "thread_scan_s": {str(k): round(v, 3) for k, v in scan.items()},
            "pinning": {k: os.environ.get(k) for k in ("OMP_PROC_BIND", "OMP_PLACES")},
            "kind": "port", "threads_tried": cands,
            "sample": f"oracle graph in stock torch-CPU ops (oneDNN/MKL; sampler end-to-end in torch), text->mel, B={Bf} x {PHONEMES * DUR} frames (padded {FRAMES_PAD}), "
                      f"T={N_STEPS} (the GPU step's own batch), OpenMP workers pinned one per core, thread count chosen on this batch from {cands} "
                      f"(`thread_scan_s`: one pass each), `value` = best of 5 passes at that count ({dt:.2f} s), `median_value` = their median ({med:.2f} s)"}


def _cpu_slice_worker(threads, lo, hi, passes):
    """One process of the multi-process CPU baseline (started by cpu_baseline_multiprocess with its core set already in force and
    OMP_NUM_THREADS set, BEFORE torch / OpenMP initialise): utterances [lo, hi) of the GPU step's batch; every pass starts when the
    parent writes a line to stdin; prints `t0 t1 frames` (CLOCK_MONOTONIC) per pass."""
    torch.set_num_threads(threads)
    from oracle import cmtts_oracle as O
    O.set_backend("torch")
    cfg = get_config("LJSpeech")
    sd = synth_cmtts_state_dict(cfg, seed=0, dur_frames=float(DUR), dur_spread=0.0)
    rs = np.random.RandomState(0)
    texts_f = rs.randint(1, cfg.n_symbols, size=(BATCH, PHONEMES)).astype(np.int64)[lo:hi]
    lens_f = np.full((hi - lo,), PHONEMES, np.int64)
    noise_f = [rs.standard_normal(size=(BATCH, 1, FRAMES_PAD, cfg.n_mels)).astype(np.float32)[lo:hi] for _ in range(N_STEPS + 1)]
    O.synthesize(sd, cfg, texts_f[:1, :8], np.asarray([8]), None, 1, [noise_f[0][:1, :, :48]])      # warm the BLAS threads
    print("ready", flush=True)
    for _ in range(passes):
        sys.stdin.readline()
        t0 = time.monotonic()
        mel, mel_len, _ = O.synthesize(sd, cfg, texts_f, lens_f, None, N_STEPS, noise_f, max_mel_len=FRAMES_PAD, torch_sampler=True)
        print(t0, time.monotonic(), int(mel_len.sum()), flush=True)


def cpu_baseline_multiprocess(threads_per_proc=16, passes=4):
    """The host's best on the GPU step's batch: one torch-CPU process per `threads_per_proc` PHYSICAL cores, each pinned to
    its own cores and given a contiguous slice of the batch (utterances are independent: the CPU twin of the GPU path's shard rule);
    `value` = the whole batch's frames / (last finish - first start) of the best pass (CLOCK_MONOTONIC is shared by the processes).
    A single process anti-scales beyond ~16 threads on these tensor sizes (`thread_scan_s`), which left most of a 128-core host idle."""
    import subprocess
    if not hasattr(os, "sched_setaffinity"):
        return {"skipped": "no sched_setaffinity on this platform"}
    avail = CPUS_AT_START
    # SMT siblings are numbered in the upper half on Linux: keep one hardware thread per core
    ncpu = os.cpu_count() or len(avail)
    phys = [c for c in avail if c < max(1, ncpu // 2)] if ncpu >= 32 and len(avail) == ncpu else avail
    nproc = max(1, min(len(phys) // threads_per_proc, BATCH))
    per = (BATCH + nproc - 1) // nproc
    nproc = (BATCH + per - 1) // per
    if nproc < 2:
        return {"skipped": f"{len(avail)} CPUs in the process mask at start ({len(phys)} physical cores): fewer than two {threads_per_proc}-core slices"}
    env = dict(os.environ, OMP_NUM_THREADS=str(threads_per_proc), OMP_PROC_BIND="close", OMP_PLACES="cores")
    env.pop("WORLD_SIZE", None)
    procs = []
    for i in range(nproc):
        lo, hi = i * per, min(BATCH, (i + 1) * per)
        cores = phys[i * threads_per_proc:(i + 1) * threads_per_proc]
        # the core set is in force before the interpreter imports torch: OpenMP derives its places from the mask it finds at start-up
        code = (f"import os, sys; os.sched_setaffinity(0, {cores!r}); sys.path.insert(0, {ROOT!r}); import bench; "
                f"bench._cpu_slice_worker({threads_per_proc}, {lo}, {hi}, {passes})")
        procs.append(subprocess.Popen([sys.executable, "-c", code], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                      env=env, text=True, cwd=ROOT))
    try:
        for p_ in procs:
            line = p_.stdout.readline()
            if line.strip() != "ready":
                raise RuntimeError(f"CPU slice worker did not start: {line!r}")
        res = [[] for _ in procs]
        for _ in range(passes):
            for p_ in procs:
                p_.stdin.write("go\n"); p_.stdin.flush()
            for i, p_ in enumerate(procs):
                t0, t1, fr = p_.stdout.readline().split()
                res[i].append((float(t0), float(t1), int(fr)))
    finally:
        for p_ in procs:
            try:
                p_.stdin.close()
            except OSError:
                pass
            try:
                p_.wait(timeout=60)
            except subprocess.TimeoutExpired:
                p_.kill()
    walls = [max(r[k][1] for r in res) - min(r[k][0] for r in res) for k in range(passes)]
    frames = sum(r[0][2] for r in res)
    timed_walls = walls[1:] if passes > 1 else walls          # pass 0 warms every process's allocator and primitives
    best = min(timed_walls)
    kb = walls.index(best)
    return {"value": round(frames / best, 1), "unit": "mel-frames/s", "cores": nproc * threads_per_proc, "processes": nproc,
            "threads_per_process": threads_per_proc, "passes_s": [round(w, 3) for w in walls],
            "slowest_process_s": round(max(r[kb][1] - r[kb][0] for r in res), 3),
            "fastest_process_s": round(min(r[kb][1] - r[kb][0] for r in res), 3)}


def cpu_quota_cores():
    """CPU time the container may use, in cores (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited / unknown.  On the GPU boxes of
    this pool it is 16.0 of 256 hardware threads: more than 16 busy threads are throttled, which is why one process anti-scales beyond
    16 threads there and why several pinned processes cannot beat one (measured: 8 x 16 threads 8.2 k frames/s against 10.6 k)."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(float(q) / float(per), 2)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else round(q / per, 2)
    except (OSError, ValueError):
        return None


def host_info():
    """nproc, CPU model and torch's thread count of the box the run happened on."""
    model = "?"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "cpu_model": model, "torch_threads": torch.get_num_threads(), "cpu_quota_cores": cpu_quota_cores()}


def cpu_baseline_small(cfg, sd, hcfg, hsd, threads):
    """The reference's own CPU-runnable shapes (BASELINE.json configs[0]) on the oracle graph in torch-CPU ops:
    (a) one 25-phoneme utterance, text -> mel at T = 1; (b) the HiFi-GAN generator on that utterance's 150 frames."""
    from oracle import cmtts_oracle as O
    O.set_backend("torch")
    torch.set_num_threads(threads)
    rs = np.random.RandomState(1)
    L = 25
    texts = rs.randint(1, cfg.n_symbols, size=(1, L)).astype(np.int64)
    lens = np.asarray([L], np.int64)
    noise = [rs.standard_normal(size=(1, 1, L * DUR, cfg.n_mels)).astype(np.float32)]
    best_m, best_v, mel = None, None, None
    for _ in range(4):
        t0 = time.perf_counter()
        mel, mel_len, _ = O.synthesize(sd, cfg, texts, lens, None, 1, noise, torch_sampler=True)
        d = time.perf_counter() - t0
        best_m = d if best_m is None or d < best_m else best_m
    mel_ct = np.ascontiguousarray(mel.transpose(0, 2, 1))
    for _ in range(3):
        t0 = time.perf_counter()
        O.hifigan_generator(hsd, hcfg, mel_ct)
        d = time.perf_counter() - t0
        best_v = d if best_v is None or d < best_v else best_v
    O.set_backend("numpy")
    frames = L * DUR
    audio = frames * cfg.hop_length / cfg.sampling_rate
    return {"cfg1_text_to_mel_T1": {"value": round(frames / best_m, 1), "unit": "mel-frames/s", "seconds": round(best_m, 4),
                                    "rtf": round(best_m / audio, 5), "cores": threads,
                                    "sample": f"B=1, {L} phonemes -> {frames} frames, T=1, best of 4"},
            "vocoder_b1": {"value": round(frames / best_v, 1), "unit": "mel-frames/s", "seconds": round(best_v, 4),
                           "rtf": round(best_v / audio, 5), "cores": threads,
                           "sample": f"HiFi-GAN generator, B=1 x {frames} frames (614.1 MFLOP/frame), best of 3"}}


def ragged_groups(lcfg, rank, world, device, per_bucket=8):
    """BASELINE.json configs[3] through shard.plan_shards: a GLOBAL ragged batch of world x 32 utterances (per_bucket x world
    per static frame bucket, lengths ~ U[0.5, 1] x bucket as SURVEY.md §8d prescribes, durations forced to 6 frames per
    phoneme) is bucketed and dealt over the ranks by length; returns this rank's bucket groups
    [(texts, src_lens, spk, noise, bucket, valid_frames)], the plan, the global frame counts and the utterance ids per group."""
    rs = np.random.RandomState(40)
    n_frames, phon = [], []
    for bucket in shard.FRAME_BUCKETS:
        Lmax = bucket // DUR
        prev = shard.FRAME_BUCKETS[shard.FRAME_BUCKETS.index(bucket) - 1] // DUR if bucket != shard.FRAME_BUCKETS[0] else 0
        ln = np.maximum((rs.uniform(0.5, 1.0, size=per_bucket * world) * Lmax).astype(np.int64), prev + 1)   # stays in ITS bucket
        phon += [int(v) for v in ln]
        n_frames += [int(v) * DUR for v in ln]
    plan = shard.plan_shards(n_frames, world)
    groups, ids = [], []
    for bucket, ranks in plan.items():
        mine = [i if i >= 0 else ranks[rank][0] for i in ranks[rank]]
        Lmax = bucket // DUR
        ln = np.asarray([phon[i] for i in mine], np.int64)
        tx = np.zeros((len(mine), Lmax), np.int64)
        for r, i in enumerate(mine):
            tx[r, :ln[r]] = np.random.RandomState(1000 + i).randint(1, lcfg.n_symbols, size=ln[r])
        gen = torch.Generator(device="cpu").manual_seed(7000 + bucket + rank)
        spk = torch.randn(len(mine), lcfg.external_speaker_dim, generator=gen)
        nz = torch.randn(N_STEPS + 1, len(mine), 1, bucket, lcfg.n_mels, generator=gen)
        valid = int(sum(n_frames[i] for i in ranks[rank] if i >= 0))
        groups.append((torch.from_numpy(tx).to(device), torch.from_numpy(ln).to(device), spk.to(device), nz.to(device), bucket, valid))
        ids.append(mine)
    return groups, plan, n_frames, ids


def multi_gpu_extras(args, cfg, model, step, timed_w, state, frames_rank, audio_s, rank, world, device, gather):
    """The per-config numbers an N-GPU run must carry (VERDICT r02 missing #2): T = 1 / 2 rates and RTF on the headline
    workload, BASELINE.json configs[3] (ragged LibriTTS shard: plan_shards -> bucket groups -> ONE all-gather of all buckets ->
    restore_order) and configs[4] (fp16 residual blocks + fp32 HiFi-GAN -> int16 PCM -> one all-gather of the PCM block).
    Every rank runs them (the timed regions hold barriers); all values are whole-job aggregates over the N ranks."""
    extras = {}
    for n in (1, 2):
        k = max(4, args.steps // 2)
        d = timed_w(lambda: step(n), k, 2)
        extras[f"frames_per_s_T{n}"] = round(frames_rank * world * k / d, 1)
        extras[f"rtf_mel_only_T{n}"] = round((d / k) / audio_s, 6)
    # ---- configs[3]
    lcfg = get_config("LibriTTS")
    lmodel = host.CMTotalTTS(lcfg, device).load_state_dict(synth_cmtts_state_dict(lcfg, seed=1, dur_frames=float(DUR), dur_spread=0.0))
    groups, plan, n_frames, ids = ragged_groups(lcfg, rank, world, device)
    bsyn = host.BucketedSynthesizer(lmodel, N_STEPS, n_streams=4)
    coll3 = host.collate_groups([g[:5] for g in groups], device)      # the shard's collate (input preparation, once): one phoneme-level call for all buckets

    def step_cfg3():
        outs = bsyn.run(coll3)
        local = {g[4]: o for g, o in zip(groups, outs)}
        state["cfg3"] = shard.allgather_buckets(local, force=gather)

    step_cfg3()
    torch.cuda.synchronize()
    host.check_async_error()
    utts = shard.restore_order(state["cfg3"], plan, len(n_frames))
    assert [int(u.shape[0]) for u in utts] == n_frames, "configs[3]: restored utterance lengths differ from the plan"
    assert all(bool(torch.isfinite(u).all()) for u in utts[:: max(1, len(utts) // 8)])
    k = max(4, args.steps // 2)
    d = timed_w(step_cfg3, k, 2)
    extras["configs3_ragged_bucketed"] = {
        "frames_per_s": round(sum(n_frames) * k / d, 1), "ms_per_step": round(d / k * 1e3, 3),
        "rtf_mel_only": round((d / k) / (sum(n_frames) * lcfg.hop_length / lcfg.sampling_rate), 6),
        "workload": f"LibriTTS model, {len(n_frames)} utterances ({len(n_frames) // world} per GPU), lengths ~ U[0.5,1] x bucket clipped to the bucket's own range, static frame "
                    f"buckets {list(shard.FRAME_BUCKETS)}, T=4, fp32; plan_shards -> bucket groups -> one all-gather of all buckets -> restore_order",
        "valid_frames": int(sum(n_frames))}
    del bsyn, groups, lmodel
    # ---- configs[4]: end-to-end wav, fp16 residual blocks + fp32 vocoder, 16 utterances x 1024 frames per GPU
    B5, L5, T5 = 16, 170, 1024
    zmodel = host.CMTotalTTS(lcfg, device).load_state_dict(synth_cmtts_state_dict(lcfg, seed=2, dur_frames=float(DUR), dur_spread=0.0))
    zmodel.set_precision("fp16")
    hcfg = HifiGanConfig()
    voc = host.Generator(hcfg, device).load_state_dict(synth_hifigan_state_dict(hcfg, seed=0))
    rs5 = np.random.RandomState(50 + rank)
    tx5 = torch.from_numpy(rs5.randint(1, lcfg.n_symbols, size=(B5, L5)).astype(np.int64)).to(device)
    ln5 = torch.full((B5,), L5, dtype=torch.int64, device=device)
    spk5 = torch.randn(B5, lcfg.external_speaker_dim, generator=torch.Generator().manual_seed(60 + rank)).to(device)

    def step_cfg4():
        o = zmodel.duration_pitch_energy_net(None, tx5, ln5, spker_embeds=spk5, max_mel_len=T5)
        nz = torch.randn(N_STEPS + 1, B5, 1, T5, lcfg.n_mels, device=device)
        mel = host.sample_with_cond(zmodel, o["cond_ct"], o["speaker_emb"], N_STEPS, nz, factors=o.get("cond_factors"))
        pcm = host.vocoder_infer_device(mel.transpose(1, 2).contiguous(), voc)
        state["cfg4"] = shard.allgather_pcm(pcm, o["mel_lens"] * lcfg.hop_length, force=gather)
        state["cfg4_local"] = pcm

    step_cfg4()
    torch.cuda.synchronize()
    host.check_async_error()
    g_pcm, g_len = state["cfg4"]
    assert g_pcm.shape == (world * B5, T5 * lcfg.hop_length) and (g_len == L5 * DUR * lcfg.hop_length).all()
    assert torch.equal(g_pcm[rank * B5:(rank + 1) * B5], state["cfg4_local"])
    k = 3
    d = timed_w(step_cfg4, k, 1)
    f5 = B5 * L5 * DUR * world
    extras["configs4_end_to_end_wav"] = {
        "frames_per_s": round(f5 * k / d, 1), "ms_per_step": round(d / k * 1e3, 3),
        "rtf_end_to_end": round((d / k) / (f5 * lcfg.hop_length / lcfg.sampling_rate), 6),
        "workload": f"LibriTTS-trained model with external speaker vectors (zero-shot input), {B5} utterances x {L5 * DUR} frames (padded {T5}) "
                    "per GPU, T=4, fp16 residual-block operands, fp32 HiFi-GAN, int16 PCM collated by one all-gather (shard.allgather_pcm)"}
    return extras


def config_blocks(device, voc, extras):
    """BASELINE.json configs[2] / [3] / [4] at THEIR OWN shapes on one GPU (the per-GPU share of the 8-GPU ones), so that the driver's record
    carries them (the table tools/config_bench.py prints): valid mel-frames/s, ms per pass and RTF = wall / audio seconds."""
    out = {}

    def clock(fn, n, warm=2):
        return timed(fn, n, warm, 1) / n

    def block(frames, d, workload, hop=256, sr=22050):
        return {"frames_per_s": round(frames / d, 1), "ms_per_pass": round(d * 1e3, 3), "rtf": round(d / (frames * hop / sr), 6),
                "valid_frames": int(frames), "workload": workload}

    def to_pcm(mel):
        return host.vocoder_infer_device(mel.transpose(1, 2).contiguous(), voc)

    def batch(cfg, B, L, seed):
        rs = np.random.RandomState(seed)
        tx = torch.from_numpy(rs.randint(1, cfg.n_symbols, size=(B, L)).astype(np.int64)).to(device)
        ln = torch.full((B,), L, dtype=torch.int64, device=device)
        spk = torch.randn(B, cfg.external_speaker_dim, generator=torch.Generator().manual_seed(seed)).to(device)
        return tx, ln, spk

    # configs[2]: VCTK multi-speaker B=64, 80x512, T=2, bf16 residual blocks (+ the universal vocoder with bf16 ResBlock convs)
    vcfg = get_config("VCTK")
    vm = host.CMTotalTTS(vcfg, device).load_state_dict(synth_cmtts_state_dict(vcfg, seed=0, dur_frames=float(DUR), dur_spread=0.0))
    tx, ln, spk = batch(vcfg, 64, PHONEMES, 3)
    nz = torch.randn(3, 64, 1, FRAMES_PAD, vcfg.n_mels, device=device)

    def c2(wav):
        o = vm.duration_pitch_energy_net(None, tx, ln, spker_embeds=spk, max_mel_len=FRAMES_PAD)
        mel = host.sample_with_cond(vm, o["cond_ct"], o["speaker_emb"], 2, nz, factors=o.get("cond_factors"))
        return to_pcm(mel) if wav else mel
    fr = 64 * PHONEMES * DUR
    vm.set_precision("bf16"); voc.set_precision("bf16")
    try:
        out["configs2_text_to_mel"] = block(fr, clock(lambda: c2(False), 8), "VCTK model, B=64, 80x512, T=2, bf16 residual-block operands (fp32 text side), text -> mel")
        out["configs2_text_to_wav"] = block(fr, clock(lambda: c2(True), 3, 1), "the same + HiFi-GAN with bf16 ResBlock convs, text -> int16 PCM")
    finally:
        vm.set_precision("fp32"); voc.set_precision("fp32")
    del vm, nz
    # configs[3]: one rank's shard (4 buckets x 8 ragged utterances, T=4, fp32) is timed above with the collated one-launch form
    if "frames_per_s_T4_libritts_bucketed_shard_one_launch" in extras:
        out["configs3_shard_text_to_mel"] = {"frames_per_s": extras["frames_per_s_T4_libritts_bucketed_shard_one_launch"],
                                             "workload": "LibriTTS model, one rank's shard of configs[3]: 4 frame buckets x 8 ragged utterances, T=4, fp32, collated text side + "
                                                         "one persistent launch per evaluation (cmtts_sample_ragged); across ranks + one all-gather of all buckets"}
    # configs[4]: zero-shot Lib -> VCTK, 16 utterances x 1024 frames per GPU, T=4, fp16 residual blocks + fp32 vocoder, end-to-end wav
    lcfg = get_config("LibriTTS")
    lm = host.CMTotalTTS(lcfg, device).load_state_dict(synth_cmtts_state_dict(lcfg, seed=2, dur_frames=float(DUR), dur_spread=0.0))
    tx, ln, spk = batch(lcfg, 16, 170, 5)
    nz = torch.randn(5, 16, 1, 1024, lcfg.n_mels, device=device)

    def c4(wav):
        o = lm.duration_pitch_energy_net(None, tx, ln, spker_embeds=spk, max_mel_len=1024)
        mel = host.sample_with_cond(lm, o["cond_ct"], o["speaker_emb"], 4, nz, factors=o.get("cond_factors"))
        return to_pcm(mel) if wav else mel
    fr = 16 * 170 * DUR
    lm.set_precision("fp16")
    try:
        out["configs4_text_to_mel"] = block(fr, clock(lambda: c4(False), 8), "LibriTTS model + external speaker vectors, B=16, 80x1024, T=4, fp16 residual-block operands, text -> mel")
        out["configs4_text_to_wav"] = block(fr, clock(lambda: c4(True), 3, 1), "the same + fp32 HiFi-GAN, text -> int16 PCM (end-to-end wav throughput)")
    finally:
        lm.set_precision("fp32")
    host.check_async_error()
    return out


def dump_outputs(out_dir, arrays):
    """Write each array as <out_dir>/<name>.npy: floating arrays as float32, integer arrays as float64 (exact for the
    lengths and indices dumped here).  Arrays past DUMP_LIMIT_BYTES are replaced by a fixed, seeded sample of their
    flattened elements (<name>.npy) and the sample's flat indices (<name>_index.npy)."""
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        a = a.astype(np.float32 if np.issubdtype(a.dtype, np.floating) else np.float64)
        if total + a.nbytes > DUMP_LIMIT_BYTES:
            room = (DUMP_LIMIT_BYTES - total) // (2 * 8)        # value + index, at most 8 bytes each
            if room <= 0:
                raise ValueError(f"--dump-outputs: no room left for {name!r} within {DUMP_LIMIT_BYTES} bytes")
            idx = np.sort(np.random.RandomState(0).choice(a.size, size=min(room, a.size), replace=False)).astype(np.float64)
            a = a.reshape(-1)[idx.astype(np.int64)]
            np.save(os.path.join(out_dir, name + "_index.npy"), idx)
            total += idx.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)
        total += a.nbytes
    return total


def self_launch(args, argv):
    """`python bench.py --gpus N` with N > 1 and no rendezvous in the environment starts the N ranks ITSELF (one process per GPU
    through torch.distributed.run on 127.0.0.1) and returns their exit code; under torch.distributed.run (WORLD_SIZE set: the
    driver's form) it checks that the launcher's world size IS --gpus and returns None.  A plain `python bench.py --gpus 8` can
    therefore never measure one GPU and print n_gpus = 8 (VERDICT r03 missing #1).  The reference has no inference launcher
    (synthesize.py:32,43 is single-process): this is the repo's own."""
    import subprocess
    n = args.gpus
    if n < 1:
        log(f"bench.py: --gpus {n} is not a GPU count")
        return 2
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != n:
            log(f"bench.py: --gpus {n} but the launcher started WORLD_SIZE={ws} ranks; refusing to report a mislabelled number "
                f"(launch with --nproc-per-node {n}, or run `python bench.py --gpus {n}` and let it launch the ranks)")
            return 2
        return None
    if n == 1:
        return None
    dry = os.environ.get("CMTTS_BENCH_DRYRUN") == "1"
    if not dry:
        have = torch.cuda.device_count()
        if have < n:
            log(f"bench.py: --gpus {n} but only {have} GPU(s) are visible on this node; nothing was measured")
            return 2
    import socket
    with socket.socket() as sk:         # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    log("bench.py: launching", " ".join(cmd))
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("OMP_PROC_BIND", None)      # set above for the single-process CPU baseline only
    env.pop("OMP_PLACES", None)
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world):
    """Launcher rehearsal without GPUs: every rank joins a gloo group, the ranks count themselves with one all-reduce and rank 0
    prints the JSON line's launcher fields."""
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        seen = dist.get_world_size()
        assert int(t.item()) == seen
        dist.barrier()
        dist.destroy_process_group()
    else:
        seen = 1
    if rank == 0:
        emit_json({"dry_run": True, "n_gpus": seen, "requested": args.gpus, "launcher": "self" if os.environ.get("TORCHELASTIC_RUN_ID") else "external"})
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure extras, roofline_16bit and cpu_baseline (each in runs of its own)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out cpu_baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: leave out extras and roofline_16bit")
    ap.add_argument("--unfused", action="store_true", help="three-launch residual block (A/B)")
    ap.add_argument("--per-layer", action="store_true", help="one fused launch per residual layer instead of the persistent stack (A/B)")
    ap.add_argument("--tile", type=int, default=0, help="frames per workgroup of the fused residual block (tuning)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (mel, lengths, durations, pitch, energy) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rc = self_launch(args, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get("CMTTS_BENCH_DRYRUN") == "1":      # launcher rehearsal (tests/test_bench_launcher.py): rendezvous only, no GPU work
        sys.exit(dry_run(args, rank, world))
    quiet_stdout()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    torch.cuda.manual_seed(DEVICE_SEED + rank)      # the in-step noise: the same draws from run to run (torch's default seed is not fixed)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=device)
        world = torch.distributed.get_world_size()       # n_gpus in the JSON line = the ranks RCCL actually joined

    cfg = get_config("LJSpeech")
    sd = synth_cmtts_state_dict(cfg, seed=0, dur_frames=float(DUR), dur_spread=0.0)
    model = host.CMTotalTTS(cfg, device).load_state_dict(sd)
    texts, lens, noise = make_inputs(cfg, rank, device)
    lib = _lib.load()
    if args.unfused:
        lib.cmtts_set_fused_resblock(0)
    if args.per_layer:
        lib.cmtts_set_persistent_denoiser(0)
    if args.tile:
        _lib.check(lib.cmtts_set_resblock_tile(args.tile))
    if os.environ.get("CMTTS_COOPERATIVE") in ("0", "1", "2"):    # A/B: persistent launches plain / cooperative / automatic (default)
        lib.cmtts_set_option(b"cooperative_launch", int(os.environ["CMTTS_COOPERATIVE"]))
    if os.environ.get("CMTTS_BRANCH_STREAMS") in ("0", "1"):      # A/B of the library's side streams
        lib.cmtts_set_option(b"branch_streams", int(os.environ["CMTTS_BRANCH_STREAMS"]))
    state = {}

    gather = world > 1 or os.environ.get("CMTTS_FORCE_COLLECTIVE") == "1"
    if gather and world == 1:          # single-GPU check of the RCCL call sequence (tools / tests, not the default run)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=device)

    def flush():
        """Complete the all-gather still in flight: the collated block of the previous batch."""
        pend = state.pop("pending", None)
        if pend is not None:
            state["gathered"], state["gathered_len"] = pend.wait()

    def step(n_steps=N_STEPS, fixed_noise=None):
        # the text side of this batch runs while RCCL collates the previous batch's mels over xGMI
        out = model.duration_pitch_energy_net(None, texts, lens, max_mel_len=FRAMES_PAD)
        flush()       # the persistent denoiser needs every CU: RCCL's kernels must be off the GPU before it starts
        # the sampler's noise is drawn INSIDE the step, on the device, like the reference does (karras_diffusion.py:534,852:
        # generator.randn / randn_like per sampling call): x_T and one draw per re-noising
        nz = fixed_noise if fixed_noise is not None else \
            torch.randn(n_steps + 1 if n_steps > 1 else 1, BATCH, 1, FRAMES_PAD, cfg.n_mels, device=device)
        mel = host.sample_with_cond(model, out["cond_ct"], None, n_steps, nz, factors=out.get("cond_factors"))
        if gather:
            state["pending"] = shard.allgather_mels_async(mel, out["mel_lens"], force=True)
        state["mel"], state["mel_len"] = mel, out["mel_lens"]
        # the text side's per-utterance outputs (small; not cond_ct and its factors, so no step keeps the previous one's buffers alive)
        state["text_out"] = {"log_d_predictions": out["log_d_predictions"], "d_rounded": out["d_rounded"], "mel2ph": out["mel2ph"],
                             "f0_denorm": out["p_predictions"]["f0_denorm"], "p_idx": out["p_predictions"]["p_idx"],
                             "e_predictions": out["e_predictions"], "e_idx": out["e_idx"]}

    step()
    flush()
    torch.cuda.synchronize()
    if gather:     # rank order, every rank's block present
        G = state["gathered"]
        assert G.shape[0] == world * BATCH and torch.equal(G[rank * BATCH:(rank + 1) * BATCH], state["mel"])
        assert (state["gathered_len"] == PHONEMES * DUR).all()
    mel_len = state["mel_len"].cpu().numpy()
    assert (mel_len == PHONEMES * DUR).all(), mel_len
    frames_rank = int(mel_len.sum())
    assert torch.isfinite(state["mel"]).all()

    # ---- headline: timed region with HIP events around the dominant kernel
    # persistent mode: ONE launch runs all residual layers of a sampler step (4 launches per step: bracket them all)
    persistent = (not args.unfused) and lib.cmtts_set_persistent_denoiser(-1) != 0 and BATCH * ((FRAMES_PAD + 63) // 64) * 2 > 256
    # persistent launches: every third one is bracketed (3 is coprime to the 4 evaluations of a step: all sigmas are sampled; a pair of event records
    # per launch put ~10 us of barrier packets around every evaluation of the timed step)
    stride = 3 if persistent else PROFILE_STRIDE
    dt = timed(step, args.steps, args.warmup, world, flush=flush,
               before=lambda: _lib.check(lib.cmtts_profile_begin(args.steps * N_STEPS * cfg.res_layers, stride)))
    tot_ms, n_l = C.c_double(), C.c_int()
    _lib.check(lib.cmtts_profile_end(C.byref(tot_ms), C.byref(n_l)))
    if args.dump_outputs and rank == 0:
        # what the last timed step handed its caller: the mels (every rank's, collated, when they are gathered) and the text side's
        # per-utterance outputs of this rank's batch
        dump_outputs(args.dump_outputs, dict({"mel": state["gathered"] if gather else state["mel"],
                                              "mel_lens": state["gathered_len"] if gather else state["mel_len"]}, **state["text_out"]))
    frames_total = frames_rank * world * args.steps
    value = frames_total / dt
    ms_per_step = dt / args.steps * 1e3
    audio_s = frames_rank * world * cfg.hop_length / cfg.sampling_rate
    C_ = cfg.res_channels
    wino, pw, wform = False, 0, ""
    if args.unfused:   # the timed kernel is the gated k=3 conv alone
        kname = "conv1d_mfma_kernel<128,128,2,2,GATED> (denoiser k=3 gated conv)"
        flops_launch = 2.0 * (2 * C_) * (3 * C_) * BATCH * FRAMES_PAD
    elif persistent:   # all residual layers of one sampler step in one launch
        # ALGORITHMIC work: the reference's convolution (3 taps x C inputs per output of the gated conv, model/blocks.py:672) — what `achieved`
        # and `frac` are priced on, whatever algorithm the kernel runs.  Since round 4 the fp32 stack's conv is a Winograd F(2,3) convolution
        # (4 products per pair of frames instead of 6): the MFMA work actually issued is reported next to it as `executed_*`.
        # Round 5: F(4,3) — 6 products per quad of frames instead of 12 (persist_wino = 3, the default; 1 / 2 = F(2,3)).
        mw = model.set_option("winograd", -1)      # model option: 1 = F(4,3) (default), 2 = F(2,3), 0 = direct
        pw = _lib.internal_set(b"persist_wino", -1) if mw else 0
        if pw == 3 and mw == 2:
            pw = 1
        wino = pw in (1, 2, 3)
        wform = {0: "", 1: "F(2,3)", 2: "F(2,3)", 3: "F(4,3)"}[pw]
        taps_issued = {0: 3.0, 1: 2.0, 2: 2.0, 3: 1.5}[pw]      # MFMA products issued per output of the k = 3 conv, in units of C inputs
        kname = (f"denoiser_persist_kernel<{'WINO ' + wform if wino else 'direct'}> ({cfg.res_layers} residual layers: gated k=3 conv"
                 f"{' as Winograd ' + wform if wino else ''} + output projection each, x / skip "
                 f"{'L2-resident between layers' if wino else 'resident in registers'}; skip head in the tail)")
        flops_launch = (2.0 * (2 * C_) * (3 * C_ + C_) * cfg.res_layers + 2.0 * C_ * (C_ + cfg.n_mels)) * BATCH * FRAMES_PAD
        flops_exec = ((2.0 * (2 * C_) * (taps_issued * C_ + C_)) * cfg.res_layers + 2.0 * C_ * (C_ + cfg.n_mels)) * BATCH * FRAMES_PAD
    else:              # fused residual block: gated k=3 conv + output projection (cp is precomputed)
        kname = "resblock_fused_kernel (gated k=3 conv + output projection of one residual layer)"
        flops_launch = 2.0 * (2 * C_) * (3 * C_ + C_) * BATCH * FRAMES_PAD
    traffic, pmc_cal, pmc_commit, pmc = None, (1.0, 1.0), "?", {}
    try:   # PMC counters cannot be sampled from inside the process: use the committed rocprofv3 pass of this workload
        pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        pmc = pj[(("denoiser_persist_kernel_wino43" if pw == 3 else "denoiser_persist_kernel_wino") if wino else "denoiser_persist_kernel") if persistent else "resblock_fused_kernel"]
        if not args.unfused and pmc["B"] == BATCH and pmc["T"] == FRAMES_PAD:
            traffic = pmc["bytes_per_launch"]
            pmc_cal = (pj["calibration"]["dword_4B_per_lane"]["fetch_factor"], pj["calibration"]["dword_4B_per_lane"]["write_factor"])
            # the ENTRY's own commit (the counters of this kernel), the calibration's beside it
            pmc_commit = "%s (counters); %s (calibration)" % (pmc.get("commit") or pmc.get("commit_r04w") or pmc.get("commit_r04") or "?", pj.get("commit", "?"))
        else:
            pmc = {}
    except Exception:
        pmc = {}
    avg_ms = tot_ms.value / max(n_l.value, 1)
    achieved = flops_launch / (avg_ms * 1e-3) / 1e12 if n_l.value else 0.0
    result = {
        "metric": "mel-frames/s (text->mel hot path, consistency sampling T=4)",
        "value": round(value, 1), "unit": "mel-frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[1]: LJSpeech model, batch 32/GPU, 80x512 mels "
                               f"({PHONEMES} phonemes x {DUR} frames = {PHONEMES * DUR} valid), T=4, fp32",
                   "batch_per_gpu": BATCH, "frames_padded": FRAMES_PAD, "sampler_steps": N_STEPS,
                   "parallelism": f"dp{world} (utterance shards + one all-gather)"},
        "rtf_mel_only": round((dt / args.steps) / audio_s, 6),
        "frames_per_s_per_gpu": round(value / world, 1),
        "padded_frames_per_s": round(BATCH * FRAMES_PAD * world * args.steps / dt, 1),
        "noise": "drawn on the device inside the timed step (torch.randn, one x_T + one draw per re-noising)",
        "host": host_info(),
        "roofline": {"bound": "mfma", "kernel": kname,
                     "achieved": round(achieved, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                     "traffic_note": "fabric-side bytes/launch = rocprofv3 FETCH_SIZE x %.1f + WRITE_SIZE x %.1f (separate --pmc passes of this "
                                     "workload at commit %s; the factors come from known-byte-count streams measured in the same session: "
                                     "FETCH_SIZE reads 1/2 on gfx950, profiles/pmc_traffic.json); Infinity-Cache hits are counted. Algorithmic "
                                     "%.1f MB; the excess = each layer's weight set once per XCD L2 (8 x %.0f MB), the polled 8-byte granules and, for the "
                                     "Winograd instances, the kernel-private residual stream x (16.8 MB) that every layer writes and the next re-reads "
                                     "through the Infinity Cache because it does not fit the L2s next to the weights (19 x 34 MB; requested a projection "
                                     "loop ahead of its use, so its latency is not on the critical path) -> %.3f of the 8 TB/s HBM peak" % (
                                         pmc_cal[0], pmc_cal[1], pmc_commit,
                                         (BATCH * FRAMES_PAD * (1024 * (cfg.res_layers + 1) + 8 * cfg.n_mels) if persistent else BATCH * FRAMES_PAD * 5120) / 1e6,
                                         # transformed conv weights (6 / 4 / 3 sets of [2C][C]) + the output projection, fp32, all layers
                                         ({3: 6, 1: 4, 2: 4}.get(pw, 3) + 1) * 2 * C_ * C_ * 4 * cfg.res_layers / 1e6,
                                         (traffic or 0) / max(avg_ms, 1e-9) / 1e-3 / (HBM_PEAK_GBS * 1e9)),
                     "launches": n_l.value, "avg_launch_us": round(avg_ms * 1e3, 2),
                     "flops_per_launch": flops_launch,
                     # the matrix pipe's own counters for this kernel, copied like `traffic` from the committed rocprofv3 passes of this
                     # workload (profiles/pmc_traffic.json names the tables and the commit): SQ_VALU_MFMA_BUSY_CYCLES over 1024 SIMDs x
                     # 2.4 GHz x time (nominal) and over GRBM_GUI_ACTIVE (the clock the launch actually ran at)
                     "mfma_busy": pmc.get("mfma_busy_nominal"), "mfma_busy_at_actual_clock": pmc.get("mfma_busy_actual"),
                     "effective_clock_ghz": pmc.get("effective_clock_ghz"), "counters_commit": pmc.get("commit")},
    }
    if persistent and not args.unfused:
        ex = flops_exec / (avg_ms * 1e-3) / 1e12 if n_l.value else 0.0
        # Round 6: `achieved` / `frac` are the HARDWARE's figures — the MFMA FLOPs the kernel issues over the launch time, against
        # the fp32 matrix peak (<= 1 by construction, and what `mfma_busy_at_actual_clock` measures from the counters).  The reference's
        # direct-form FLOPs (what the launch computes for the caller) are carried beside it as `algorithmic_*`; their ratio to
        # the issued count is the Winograd form's saving.
        result["roofline"].update({
            "achieved": round(ex, 2), "frac": round(ex / FP32_MFMA_PEAK_TFLOPS, 4),
            "algorithmic_flops_per_launch": flops_launch, "algorithmic_tflops": round(achieved, 2),
            "algorithmic_frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "algorithmic_speedup": round(flops_launch / flops_exec, 3),
            "algorithm": (f"Winograd {wform} along the frame axis for the gated k=3 conv (fp32 transforms, weights transformed in double and rounded once; "
                          f"|d mel| ~{'8e-6' if pw == 3 else '4e-6'} against the direct form, tests/test_gpu_precision.py), direct 1x1 output projection" if wino else "direct"),
            "executed_flops_per_launch": flops_exec, "executed_tflops": round(ex, 2),
            "executed_frac": round(ex / FP32_MFMA_PEAK_TFLOPS, 4),
            "frac_note": "`achieved` / `frac` = the MFMA FLOPs actually ISSUED per launch (`executed_*`, the same numbers) over the launch time and the fp32 matrix peak: the "
                         "matrix pipe's own duty, which `mfma_busy*` measures from the counters.  `algorithmic_*` = the reference's direct-form FLOPs (SURVEY.md 8(d)) over "
                         "the same time: with the Winograd form the kernel issues only 1/2 (F(4,3)) or 2/3 (F(2,3)) of the conv's multiplies, so `algorithmic_frac` can exceed "
                         "1.0 without the hardware exceeding its peak (`algorithmic_speedup` = direct-form / issued FLOPs)"})

    # ---- --full only: everything below runs after the headline's timed steps and dump, in runs of its own
    extras_on = args.full and not args.no_extras
    if (world > 1 or gather or os.environ.get("CMTTS_MULTI_EXTRAS") == "1") and extras_on:      # gather: CMTTS_FORCE_COLLECTIVE=1 on one GPU
        # every rank takes part: T = 1 / 2, configs[3] and configs[4] with their collectives (whole-job aggregates)
        result["extras"] = multi_gpu_extras(args, cfg, model, step, lambda f, k, w: timed(f, k, w, world, flush=flush), state,
                                            frames_rank, audio_s, rank, world, device, gather)
        flush()
    if rank == 0 and world == 1 and extras_on:
        extras = result.get("extras", {})
        for n in (1, 2):
            k = max(4, args.steps // 2)
            d = timed(lambda: step(n), k, 2, 1)
            extras[f"frames_per_s_T{n}"] = round(frames_rank * k / d, 1)
            extras[f"rtf_mel_only_T{n}"] = round((d / k) / audio_s, 6)
        # throughput mode: conditioning of batch i+1 on a second HIP stream under the sampler of batch i
        pipe = host.StreamPipelinedSynthesizer(model, N_STEPS)
        nxt = (texts, lens, None, FRAMES_PAD)
        pipe.prepare(*nxt)

        def step_pipelined():
            state["mel_p"], _ = pipe.sample_and_prepare_next(noise, nxt)
        k = args.steps
        d = timed(step_pipelined, k, 3, 1)
        torch.cuda.synchronize()
        step(fixed_noise=noise)
        torch.cuda.synchronize()
        assert torch.equal(state["mel_p"], state["mel"]), "pipelined result differs"
        extras["frames_per_s_T4_two_stream_pipeline"] = round(frames_rank * k / d, 1)
        # reduced-precision denoiser operands (BASELINE.json configs[2]/[4]); NOT the headline (fp32)
        for dt in ("bf16", "fp16", "fp16x3"):
            model.set_precision(dt)
            k = max(4, args.steps // 2)
            d = timed(step, k, 2, 1)
            extras[f"frames_per_s_T4_{dt}_resblocks"] = round(frames_rank * k / d, 1)
            if dt != "fp16x3":     # + the opt-in 16-bit FFN contractions of the text encoder (set_option("text16", 1): the integer stages then depend on the mode)
                model.set_option("text16", 1)
                d = timed(step, k, 2, 1)
                model.set_option("text16", 0)
                extras[f"frames_per_s_T4_{dt}_resblocks_text16"] = round(frames_rank * k / d, 1)
        model.set_precision("fp32")
        extras["fp16x3_note"] = ("residual-block operands as hi + lo fp16 pairs (22 bits), three fp16 MFMAs per product, fp32 accumulate: "
                                 "fp32-class accuracy (tests/test_gpu_precision.py: error vs float64 within 2x of the exact-fp32 kernels'); "
                                 "exploratory — the headline `value` is the exact-fp32 path")
        # north-star shape: 80x1024 frames per utterance (BASELINE.json north_star), same batch of 32, T=4
        L2, T2 = 171, 1024
        rs2 = np.random.RandomState(99)
        texts2 = torch.from_numpy(rs2.randint(1, cfg.n_symbols, size=(BATCH, L2)).astype(np.int64)).to(device)
        lens2 = torch.full((BATCH,), L2, dtype=torch.int64, device=device)
        noise2 = torch.randn(N_STEPS + 1, BATCH, 1, T2, cfg.n_mels, device=device)

        def step1024():
            o = model.duration_pitch_energy_net(None, texts2, lens2, max_mel_len=T2)
            state["mel1024"] = host.sample_with_cond(model, o["cond_ct"], None, N_STEPS, noise2, factors=o.get("cond_factors"))
        k = max(4, args.steps // 2)
        d = timed(step1024, k, 2, 1)
        extras["frames_per_s_T4_80x1024"] = round(BATCH * T2 * k / d, 1)      # frames truncated to the 1024 bucket
        del noise2
        # BASELINE.json configs[3] shape on one rank: LibriTTS (multi-speaker) model, a 32-utterance shard of ragged
        # lengths dealt into static frame buckets (256 / 512 / 768 / 1024, 8 utterances each), T=4, fp32
        lcfg = get_config("LibriTTS")
        lmodel = host.CMTotalTTS(lcfg, device).load_state_dict(synth_cmtts_state_dict(lcfg, seed=1, dur_frames=float(DUR), dur_spread=0.0))
        rs4 = np.random.RandomState(4)
        groups = []
        for bucket in shard.FRAME_BUCKETS:
            n = 8
            Lmax = bucket // DUR
            ln = np.maximum((rs4.uniform(0.5, 1.0, size=n) * Lmax).astype(np.int64), 1)
            ln[0] = Lmax
            tx = rs4.randint(1, lcfg.n_symbols, size=(n, Lmax)).astype(np.int64)
            tx[np.arange(Lmax)[None, :] >= ln[:, None]] = 0
            gen4 = torch.Generator(device="cpu").manual_seed(bucket)
            groups.append((torch.from_numpy(tx).to(device), torch.from_numpy(ln).to(device),
                           torch.randn(n, lcfg.external_speaker_dim, generator=gen4).to(device),
                           torch.randn(N_STEPS + 1, n, 1, bucket, lcfg.n_mels, generator=gen4).to(device), bucket, int(ln.sum()) * DUR))

        def step_bucketed():
            for tx, ln, spk, nz, bucket, _ in groups:
                o = lmodel.duration_pitch_energy_net(None, tx, ln, spker_embeds=spk, max_mel_len=bucket)
                state["mel_b"] = host.sample_with_cond(lmodel, o["cond_ct"], o["speaker_emb"], N_STEPS, nz, factors=o.get("cond_factors"))
        k = max(4, args.steps // 2)
        d = timed(step_bucketed, k, 2, 1)
        extras["frames_per_s_T4_libritts_bucketed_shard"] = round(sum(g[5] for g in groups) * k / d, 1)   # valid frames only
        bsyn = host.BucketedSynthesizer(lmodel, N_STEPS, n_streams=4, mode="streams")      # one HIP stream per bucket group

        def step_bucketed_streams():
            state["mel_b"] = bsyn.run([g[:5] for g in groups])
        d = timed(step_bucketed_streams, k, 2, 1)
        extras["frames_per_s_T4_libritts_bucketed_shard_4_streams"] = round(sum(g[5] for g in groups) * k / d, 1)
        # round 3: the text side of the groups on four streams, then ALL groups' residual layers in one persistent launch per
        # evaluation (cmtts_sample_ragged), utterances trimmed to mel_len + 16 frames + the sampler's receptive field
        bsyn = host.BucketedSynthesizer(lmodel, N_STEPS, n_streams=4, mode="ragged", tail_frames=16, batch_text=False)
        d = timed(step_bucketed_streams, k, 2, 1)
        extras["frames_per_s_T4_libritts_bucketed_shard_one_launch_text_per_group"] = round(sum(g[5] for g in groups) * k / d, 1)    # round 3's form
        # round 4: the phoneme-level half of ALL groups in one call as well (cmtts_text_forward_ragged on the collated shard), the
        # conditioner projections expanded from their factors
        coll = host.collate_groups([g[:5] for g in groups], device)
        bsyn = host.BucketedSynthesizer(lmodel, N_STEPS, n_streams=4, mode="ragged", tail_frames=16)

        def step_collated():
            state["mel_b"] = bsyn.run(coll)
        d = timed(step_collated, k, 2, 1)
        extras["frames_per_s_T4_libritts_bucketed_shard_one_launch"] = round(sum(g[5] for g in groups) * k / d, 1)
        bsyn = host.BucketedSynthesizer(lmodel, N_STEPS, n_streams=4, mode="ragged", trim=False)
        d = timed(step_collated, k, 2, 1)
        extras["frames_per_s_T4_libritts_bucketed_shard_one_launch_untrimmed"] = round(sum(g[5] for g in groups) * k / d, 1)
        del coll
        del bsyn
        del groups, lmodel
        # end to end with the HiFi-GAN generator (fp32), T=4
        hcfg = HifiGanConfig()
        voc = host.Generator(hcfg, device).load_state_dict(synth_hifigan_state_dict(hcfg, seed=0))

        def e2e():
            step()
            state["wav"] = voc(state["mel"].transpose(1, 2).contiguous())
        k = 3
        d = timed(e2e, k, 1, 1)
        assert torch.isfinite(state["wav"]).all()
        extras["frames_per_s_end_to_end_wav_T4"] = round(frames_rank * k / d, 1)
        extras["rtf_end_to_end_T4"] = round((d / k) / audio_s, 6)
        # the reference's own RTF (p_rtf_cm.py:191-230): the clock starts AFTER the duration net and covers the sampler +
        # vocoder of the whole batch; the denominator is the FIRST utterance's duration only
        out_r = model.duration_pitch_energy_net(None, texts, lens, max_mel_len=FRAMES_PAD)
        first_s = float(out_r["mel_lens"][0].item()) * cfg.hop_length / cfg.sampling_rate

        def ref_style(n_steps):
            nz = torch.randn(n_steps + 1 if n_steps > 1 else 1, BATCH, 1, FRAMES_PAD, cfg.n_mels, device=device)
            m_ = host.sample_with_cond(model, out_r["cond_ct"], None, n_steps, nz)
            state["wav"] = voc(m_.transpose(1, 2).contiguous())
        for n in (1, 4):
            d_ = timed(lambda: ref_style(n), 3, 1, 1)
            extras[f"rtf_reference_style_T{n}"] = round((d_ / 3) / first_s, 6)
        extras["rtf_reference_style_note"] = ("p_rtf_cm.py:191-230: (sampler + vocoder time of the whole B=32 batch) / (duration of the first "
                                              "utterance); fp32 vocoder, no file I/O")
        # the vocoder alone: the end-to-end bottleneck, with its own roofline (614.1 MFLOP per mel frame, fp32 MFMA)
        mel_v = state["mel"].transpose(1, 2).contiguous()
        d_v = timed(lambda: state.__setitem__("wav", voc(mel_v)), 5, 2, 1) / 5
        vflops = 614105088.0 * BATCH * FRAMES_PAD
        wino_default = (_lib.internal_set(b"voc_wino", -1) == 1 and voc.set_option("winograd", -1) == 1 and _lib.internal_set(b"voc_wino43", -1) == 1 and
                        _lib.internal_set(b"voc_wino64", -1) == 1 and BATCH * FRAMES_PAD * 8 // 64 >= 1024)
        vx = vocoder_issued_flops_per_frame(wino_default)
        vexec = vx["flops_per_frame"] * BATCH * FRAMES_PAD
        extras["vocoder_fp32"] = {"ms_per_batch": round(d_v * 1e3, 2),
                                  # hardware figures first: the MFMA FLOPs the generator ISSUES over its time and the fp32 matrix peak
                                  "achieved_tflops": round(vexec / d_v / 1e12, 1),
                                  "frac_of_fp32_mfma_peak": round(vexec / d_v / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                                  "executed_flops_per_batch": vexec, "conv_forms": vx["forms"],
                                  # ... and the reference's direct-form FLOPs (614.1 MFLOP per mel frame) over the same time
                                  "algorithmic_tflops": round(vflops / d_v / 1e12, 1),
                                  "algorithmic_frac": round(vflops / d_v / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                                  "algorithmic_speedup": round(vflops / vexec, 3),
                                  "bound": "mfma", "flops_per_batch": vflops,
                                  "algorithm": ("ResBlock convs of the C >= 128 stages (and k >= 7 at C = 64) in a Winograd form: dilation 1 and 3 (and 5 at C = 256 or k = 3) as F(4,3) tap groups — "
                                                "6 / 16 / 24 products per quad of outputs instead of 12 / 28 / 44 — the other dilation-5 convs as F(2,3) tap groups (4 / 10 / 15 per "
                                                "pair instead of 6 / 14 / 22); |d wav| <= 1.4e-6 against the direct form; `achieved_tflops` / the fraction count the "
                                                "FLOPs issued, `algorithmic_*` the reference's direct-form FLOPs" if _lib.internal_set(b"voc_wino", -1) >= 1 and voc.set_option("winograd", -1) == 1 else "direct")}
        # BASELINE.json configs[2] shape: bf16 residual blocks + bf16 HiFi-GAN ResBlock convs (fp32 accumulate)
        model.set_precision("bf16")
        voc.set_precision("bf16")
        d = timed(e2e, k, 1, 1)
        model.set_precision("fp32")
        voc.set_precision("fp32")
        assert torch.isfinite(state["wav"]).all()
        extras["frames_per_s_end_to_end_wav_T4_bf16"] = round(frames_rank * k / d, 1)
        voc.set_precision("bf16")
        d_v = timed(lambda: state.__setitem__("wav", voc(mel_v)), 5, 2, 1) / 5
        voc.set_precision("fp32")
        extras["vocoder_bf16"] = {"ms_per_batch": round(d_v * 1e3, 2), "achieved_tflops": round(vflops / d_v / 1e12, 1),
                                  "frac_of_bf16_mfma_peak": round(vflops / d_v / 1e12 / 2500.0, 4),
                                  "note": "bf16 operands in the ResBlock convs and the upsamplers (conv_pre / conv_post fp32); whole ResBlocks / pairs at C <= 64, one-launch in-place pairs at C = 128 (round 3), X-resident convs at C = 256 (profiles/r03_16bit_paths.md)"}
        # fp16x3 everywhere (residual blocks + HiFi-GAN ResBlock convs): fp32-class accuracy, exploratory
        model.set_precision("fp16x3")
        voc.set_precision("fp16x3")
        d = timed(e2e, k, 1, 1)
        d_v = timed(lambda: state.__setitem__("wav", voc(mel_v)), 5, 2, 1) / 5
        model.set_precision("fp32")
        voc.set_precision("fp32")
        assert torch.isfinite(state["wav"]).all()
        extras["frames_per_s_end_to_end_wav_T4_fp16x3"] = round(frames_rank * k / d, 1)
        extras["vocoder_fp16x3"] = {"ms_per_batch": round(d_v * 1e3, 2), "achieved_tflops": round(vflops / d_v / 1e12, 1),
                                    "note": "fp16 hi + lo operands, three MFMAs per product (fp32-class; tests/test_gpu_precision.py)"}
        state["hifigan"] = (hcfg, synth_hifigan_state_dict(hcfg, seed=0))
        extras["configs"] = config_blocks(device, voc, extras)
        # ---- second roofline block: the 16-bit paths against the 2.5 PFLOP/s dense bf16 MFMA peak.  (a) the persistent
        # denoiser stack with bf16 operands: HIP events around its launches, like the headline's; (b) the bf16 HiFi-GAN generator as a
        # whole (its time is spread over ~40 kernel shapes: profiles/r03_16bit_paths.md has the per-kernel tables)
        BF16_PEAK = 2500.0
        model.set_precision("bf16")
        k = max(4, args.steps // 2)
        d_lp = timed(step, k, 2, 1, before=lambda: _lib.check(lib.cmtts_profile_begin(k * N_STEPS * cfg.res_layers, 1)))
        tms, nl = C.c_double(), C.c_int()
        _lib.check(lib.cmtts_profile_end(C.byref(tms), C.byref(nl)))
        model.set_precision("fp32")
        lp_us = tms.value / max(nl.value, 1) * 1e3
        lp_flops = (2.0 * (2 * C_) * (3 * C_ + C_) * cfg.res_layers + 2.0 * C_ * (C_ + cfg.n_mels)) * BATCH * FRAMES_PAD
        try:
            pj2 = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        except Exception:
            pj2 = {}
        lp_ach = lp_flops / (lp_us * 1e-6) / 1e12 if nl.value else 0.0
        vb = extras["vocoder_bf16"]
        result["roofline_16bit"] = [
            {"bound": "mfma", "kernel": "denoiser_persist_lp_kernel<bf16> (20 residual layers, bf16 operands, fp32 state / accumulate / tail)",
             "achieved": round(lp_ach, 1), "peak": BF16_PEAK, "unit": "TFLOP/s", "frac": round(lp_ach / BF16_PEAK, 4),
             "launches": nl.value, "avg_launch_us": round(lp_us, 2), "flops_per_launch": lp_flops,
             "traffic": pj2.get("denoiser_persist_lp_kernel", {}).get("bytes_per_launch"),
             "note": "bound in practice by the per-XCD L2 -> CU weight delivery (1.05 MB per workgroup per layer), not by the matrix pipe "
                     "(26 % MFMA-busy) or HBM (1.7 TB/s at the fabric): profiles/r03_16bit_paths.md"},
            {"bound": "mfma", "kernel": "HiFi-GAN generator, bf16 operands (whole forward: ~40 kernel shapes)",
             "achieved": vb["achieved_tflops"], "peak": BF16_PEAK, "unit": "TFLOP/s", "frac": round(vb["achieved_tflops"] / BF16_PEAK, 4),
             "ms_per_batch": vb["ms_per_batch"], "flops_per_batch": vflops,
             "traffic": pj2.get("vocoder_bf16", {}).get("bytes_per_batch"),
             "note": "fabric-side bytes per 32 x 512-frame batch from separate --pmc FETCH_SIZE / WRITE_SIZE passes (calibrated); the "
                     "C = 128 pairs sit at the bf16 ridge (451 FLOP/B at k = 11 against 2.5 PF / 5 TB/s = 500), the narrow stages are "
                     "bound by per-conv fixed costs: profiles/r03_16bit_paths.md"}]
        result["extras"] = extras
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(cfg, sd)
        result["cpu_baseline"]["host_cores"] = os.cpu_count()
        result["cpu_baseline"]["cpu_quota_cores"] = cpu_quota_cores()
        try:
            quota = cpu_quota_cores()
            if quota is not None and quota < 2 * 16:
                mpb = {"skipped": f"the container's CPU quota is {quota} cores (cgroup cpu.max) of {os.cpu_count()} hardware threads: a second 16-thread process "
                                  "would only be throttled (measured once on this pool: 8 x 16 pinned threads 8.2 k frames/s against 10.6 k for one process); "
                                  "the same quota is why `thread_scan_s` anti-scales beyond 16 threads"}
            else:
                mpb = cpu_baseline_multiprocess()
        except Exception as e:      # a box that cannot spawn / pin keeps the single-process figure
            mpb = {"skipped": "failed: " + repr(e)}
        if "value" not in mpb or mpb["value"] <= result["cpu_baseline"]["value"]:
            result["cpu_baseline"]["multi_process"] = mpb
        else:
            # `value` = the host's best: the multi-process figure; the single-process best of the scan stays beside it
            sp = result["cpu_baseline"]
            result["cpu_baseline"] = dict(sp, value=mpb["value"], cores=mpb["cores"], single_process_value=sp["value"], single_process_cores=sp["cores"],
                                          multi_process=mpb,
                                          sample=sp["sample"] + f"; `value` = {mpb['processes']} such processes x {mpb['threads_per_process']} pinned threads, each on a contiguous "
                                                               f"slice of the batch, whole batch / slowest process, best of {len(mpb['passes_s']) - 1} timed passes ({min(mpb['passes_s'][1:]):.2f} s); "
                                                               "`single_process_value` = the best single process of the thread scan")
        hcfg_c, hsd_c = state.get("hifigan") or (HifiGanConfig(), synth_hifigan_state_dict(HifiGanConfig(), seed=0))
        result["cpu_baseline"]["small_shapes"] = cpu_baseline_small(cfg, sd, hcfg_c, hsd_c, result["cpu_baseline"].get("single_process_cores", result["cpu_baseline"]["cores"]))
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()
    # RCCL writes a banner ("Librccl path : ...") through C stdio, which is fully buffered on a pipe and would land
    # AFTER the result at exit: drain it first so the JSON line is the last line of stdout
    C.CDLL(None).fflush(None)
    if rank == 0:
        emit_json(result)


_JSON_FD = None


def quiet_stdout():
    """stdout carries ONE JSON line (the driver's contract).  RCCL prints a version banner to fd 1 when a communicator comes up, and any
    library may: from here on fd 1 is stderr, and emit_json() writes the line to the ORIGINAL stdout."""
    global _JSON_FD
    if _JSON_FD is None:
        sys.stdout.flush()
        _JSON_FD = os.dup(1)
        os.dup2(2, 1)


def emit_json(obj):
    line = (json.dumps(obj) + "\n").encode()
    sys.stdout.flush()
    if _JSON_FD is None:
        os.write(1, line)
    else:
        os.write(_JSON_FD, line)


if __name__ == "__main__":
    main()
