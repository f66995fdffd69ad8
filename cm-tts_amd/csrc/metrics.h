// Objective metrics of a rendering against its recording (metrics.hip; include/cmtts_hip.h: cmtts_metric_*; the definition in
// executable form: cmtts_amd/metrics.py): cepstra of the log-mel, the cepstral cost matrix the DTW of align.hip takes, the path statistics
// of two F0 tracks, the column-normalised images and their structural similarity.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int MT_CH = 80;                     // mel channels, and the most cepstra / image columns
constexpr int MT_MAX_SIDE = 4096;             // frames per side
constexpr int MT_MAX_B = 65535;
constexpr int MT_WIN = 11;                    // taps of the SSIM window per axis
constexpr int MT_SSIM_ROWS = 8;               // window rows (recording frames) one workgroup of the SSIM evaluates: MT_SSIM_ROWS + 10 frames in LDS

inline int metric_ssim_tiles(int Tr) { return Tr > MT_WIN - 1 ? (Tr - (MT_WIN - 1) + MT_SSIM_ROWS - 1) / MT_SSIM_ROWS : 1; }
