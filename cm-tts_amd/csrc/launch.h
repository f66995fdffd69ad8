// What the host-side launch sequences (denoiser_side.hip: denoiser and sampler side; text_side.hip: text and frame side; vocoder.hip: the HiFi-GAN
// generator) and the rest of the C ABI (cmtts_api.hip) share: the generic conv's argument fill and launch, workspace carving, the library-owned
// side streams and the switch tables.  Like fail() in model.h: declared here, defined once in cmtts_api.hip unless noted; small things are inline.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "model.h"
#include "conv_args.h"

// A plain Conv1d over [B][cin][ldx] -> [B][cout][ldy]: "same" padding, dilation 1, no activation; callers adjust the fields that differ.
ConvArgs conv_args(const PackedConv& w, const float* X, int Tin, int ldx, long x_bs, float* Y, int ldy, long y_bs, int N);
int launch(const ConvArgs& a, int epi, int nbatch, hipStream_t s);      // the generic fp32 conv kernel (conv_mfma.hip); fail()s on error

struct Carver {      // consecutive 256-byte aligned slices of a caller-provided workspace
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T* p = (T*)(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// Library-owned side streams of a caller stream (public option "branch_streams"): independent branches of a call are forked
// from and joined back into the caller's stream with events.
struct SideStream {
    hipStream_t user, side;
    hipEvent_t fork, join;
    hipStream_t side2 = nullptr;                      // second side stream + chain events: the three ResBlocks of an MRF stage (vocoder.hip)
    hipEvent_t join2 = nullptr, done0 = nullptr, done1 = nullptr;
};
SideStream* side_for(hipStream_t s);      // null: branch_streams is off or no stream could be had — the caller runs in line
bool side2_ready(SideStream* ss);         // creates side2 / join2 / done0 / done1 on first use
int branch_fork(SideStream* ss);          // work queued on ss->side after this sees everything queued on ss->user so far
int branch_join(SideStream* ss);          // work queued on ss->user after this sees everything queued on ss->side so far

int persist_blocks();                     // workgroups that are certainly co-resident: the CU count (denoiser_side.hip)
// The phoneme-level factor of the conditioner projections, p1 [B][res_layers * res_channels][Lp] = Wc * out1 (the frame side computes it beside its
// predictors; denoiser_side.hip)
int cond_phoneme_factor(cmtts_model* m, const float* out1, int B, int Lp, float* p1, hipStream_t s);

// Host copy of an int32 table that is device or page-locked host memory: a host table is read in place, a device table is read
// back on `s`, which synchronises it.  *on_host tells which it was.  (vocoder.hip)
int fetch_table(const char* who, const void* table, void* host_copy, size_t bytes, hipStream_t s, bool* on_host);

// Named integer switches: knob_set returns the previous value (a value outside [lo, hi] only queries); *found = the name is in the table.
struct Knob { const char* name; int* var; int lo, hi; };
int knob_set(const Knob* tab, size_t n, const char* name, int value, bool* found);
int vocoder_internal_set(const char* name, int value, bool* found);      // vocoder.hip: the generator's switches, asked first by cmtts_internal_set
int text_internal_set(const char* name, int value, bool* found);         // text_side.hip: the FFT blocks', predictors' and frame side's switches, asked second
int denoiser_internal_set(const char* name, int value, bool* found);     // denoiser_side.hip: cond_*, persist_tail, persist_wino, inproj_fused, asked last
extern int g_split_resblock, g_step_cache;      // denoiser_side.hip: the variables of its two rows of cmtts_set_option (resblock_split, step_cache)
void denoiser_error_word_ready();         // denoiser_side.hip: allocates the process's pinned error word once (cmtts_finalize; cmtts_poll_error reads it)
