// Arguments of the text-state record copy (text_state.hip): the per-utterance state cmtts_frame_forward_sub reads from a text
// workspace, gathered into / scattered from fixed-size records (include/cmtts_hip.h: cmtts_text_state_*).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define TEXT_STATE_MAX_REGIONS 5
#define TEXT_STATE_HEADER_BYTES 64
#define TEXT_STATE_LAYOUT 0x54530001u      // "TS", layout revision 1: out1, h128, spk, cum
#define TEXT_STATE_LAYOUT_P 0x54530002u    // layout revision 2: revision 1 + the pitch control table's row fp32 [L_all] as a fifth region

// The record header (64 bytes, first in every record).
struct TextStateHeader {
    int64_t index;         // global utterance index
    int64_t mel_len;       // sum of the rounded durations (= cum[L_all - 1])
    int32_t src_len;
    uint32_t layout;       // TEXT_STATE_LAYOUT, or TEXT_STATE_LAYOUT_P with a pitch control table
    int32_t L_all, hidden, cwt_hidden, n_regions;
    int32_t pad[6];
};
static_assert(sizeof(TextStateHeader) == TEXT_STATE_HEADER_BYTES, "record header is 64 bytes");

// One per-utterance slab of the text workspace: utterance b's bytes start at ws + b * ws_stride.
struct TextStateRegion {
    char* ws;
    long ws_stride;        // bytes between utterances in the workspace
    long rec_off;          // byte offset inside a record (16-byte aligned)
    long bytes;            // bytes per utterance
    int vec16;             // every address and size a multiple of 16: dwordx4 copies; else dword copies
    int chunk0;            // first copy chunk of this region
};

struct TextStateCopy {
    TextStateRegion reg[TEXT_STATE_MAX_REGIONS];
    int n_regions, n_chunks;     // chunks per record (all regions)
    int unpack;                  // 0: workspace rows -> records (+ header), 1: records -> workspace rows 0..n-1
    uint32_t layout;             // pack: the header's layout word
    int n, B_all, L_all, hidden, cwt_hidden;
    char* rec;                   // records [n][rec_bytes]
    long rec_bytes;
    const int32_t* rows;         // pack: workspace row of record r (device)
    const int64_t* index;        // pack: global utterance index of record r (device; null = the row)
    const int64_t* src_lens;     // pack: [B_all] (device; null = -1 in the header)
    const int32_t* cum;          // pack: the workspace's cumulative durations [B_all][L_all] (mel_len of the header)
};

// bytes copied by one workgroup (256 lanes x 4 x 16 B)
#define TEXT_STATE_CHUNK 16384

#ifdef __cplusplus
extern "C" {
#endif
int cmtts_launch_text_state_copy(const TextStateCopy* a, void* stream);
#ifdef __cplusplus
}
#endif
