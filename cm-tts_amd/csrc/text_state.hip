// Per-utterance text-side state as fixed-size records (include/cmtts_hip.h: cmtts_text_state_pack / _unpack): the hand-off between
// the two phases of a sharded synthesis.  New work: the reference synthesizes one padded batch in one process (synthesize.py:195-227).
// Pure bandwidth: every workgroup copies one 16 KB chunk of one region of one record with dwordx4 loads (all four issued before the
// first store) and dwordx4 stores; regions whose per-utterance stride is not a multiple of 16 bytes (cum: [B][L] int32) go by dwords.
// One launch moves every region of every record.
#include <hip/hip_runtime.h>

#include "text_state.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_VEC = TEXT_STATE_CHUNK / (TS_THREADS * 16);      // 16-byte vectors per lane and chunk

__global__ __launch_bounds__(TS_THREADS) void text_state_copy_kernel(TextStateCopy a) {
    const int r = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    int row = r;
    if (!a.unpack) {
        row = a.rows[r];
        if (row < 0 || row >= a.B_all) return;           // out-of-range row: nothing read, the record stays as it was
    }
    char* rec = a.rec + (long)r * a.rec_bytes;
    if (c == a.n_chunks) {                               // pack only: the header
        if (tid == 0) {
            TextStateHeader h = {};
            h.index = a.index ? a.index[r] : row;
            h.mel_len = a.cum[(long)row * a.L_all + a.L_all - 1];
            h.src_len = a.src_lens ? (int32_t)a.src_lens[row] : -1;
            h.layout = a.layout;
            h.L_all = a.L_all; h.hidden = a.hidden; h.cwt_hidden = a.cwt_hidden; h.n_regions = a.n_regions;
            *reinterpret_cast<TextStateHeader*>(rec) = h;
        }
        return;
    }
    // the region of this chunk: every entry of the table read up front (independent scalar loads), no dependent walk
    TextStateRegion R = a.reg[0];
#pragma unroll
    for (int g = 1; g < TEXT_STATE_MAX_REGIONS; ++g)
        if (g < a.n_regions && c >= a.reg[g].chunk0) R = a.reg[g];
    const long off = (long)(c - R.chunk0) * TEXT_STATE_CHUNK;
    const long nb = R.bytes - off < TEXT_STATE_CHUNK ? R.bytes - off : TEXT_STATE_CHUNK;
    char* wsp = R.ws + (long)row * R.ws_stride + off;
    char* rp = rec + R.rec_off + off;
    const char* src = a.unpack ? rp : wsp;
    char* dst = a.unpack ? wsp : rp;
    if (R.vec16) {
        // all four loads unconditional (a lane past the end of a partial chunk re-reads the chunk's first vector), so they issue
        // back to back under one wait; only the stores are guarded
        uint4 v[TS_VEC];
#pragma unroll
        for (int k = 0; k < TS_VEC; ++k) {
            const long i = ((long)k * TS_THREADS + tid) * 16;
            v[k] = *reinterpret_cast<const uint4*>(src + (i < nb ? i : 0));
        }
#pragma unroll
        for (int k = 0; k < TS_VEC; ++k) {
            const long i = ((long)k * TS_THREADS + tid) * 16;
            if (i < nb) *reinterpret_cast<uint4*>(dst + i) = v[k];
        }
    } else {
        for (long i = (long)tid * 4; i < nb; i += TS_THREADS * 4)
            *reinterpret_cast<uint32_t*>(dst + i) = *reinterpret_cast<const uint32_t*>(src + i);
    }
}

}  // namespace

extern "C" int cmtts_launch_text_state_copy(const TextStateCopy* a, void* stream) {
    if (a->n <= 0 || a->n_chunks <= 0) return 0;
    const dim3 grid(a->n_chunks + (a->unpack ? 0 : 1), a->n);
    hipLaunchKernelGGL(text_state_copy_kernel, grid, dim3(TS_THREADS), 0, (hipStream_t)stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
