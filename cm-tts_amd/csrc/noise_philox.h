// Seeded per-utterance sampler noise (noise_philox.hip; include/cmtts_hip.h: cmtts_noise_fill, cmtts_noise_fill_groups).
#pragma once
#include <stdint.h>

// One padded (B, T) group of a ragged shard as the groups kernel takes it, by value in its arguments.
struct NoiseGroup {
    const int64_t* seeds;      // device [B]
    float* out;                // device [n_draws][B][1][T][M]
    int32_t B, T;
    int32_t wg0;               // first workgroup (grid x) of this group: filled by the launcher
    int32_t wg_per_utt;        // ceil(T * ceil(M / 4) / 256): filled by the launcher
};
constexpr int NOISE_MAX_GROUPS = 32;      // groups per launch (1 KB of kernel arguments); the launcher loops above it
struct NoiseGroupTable {
    NoiseGroup g[NOISE_MAX_GROUPS];
};

#ifdef __cplusplus
extern "C" {
#endif
// out[d][b][0][t][m] = scale * z(seeds[b], first_draw + d, t0 + t, m) for d < n_draws.  bits != nullptr: the raw Philox blocks
// uint32 [n_draws][B][T][ceil(M / 4)][4] instead (test hook; out ignored).  Arguments are NOT validated here.  0, or -3 on a launch error.
int cmtts_launch_noise_fill(const int64_t* seeds, int B, int T, int M, int first_draw, int n_draws, int64_t t0, float scale, float* out,
                            uint32_t* bits, void* stream);
// Every group of `groups` (host array; wg0 / wg_per_utt are the launcher's) in one launch per NOISE_MAX_GROUPS groups, t0 = 0, scale = 1.
int cmtts_launch_noise_fill_groups(const NoiseGroup* groups, int n_groups, int M, int first_draw, int n_draws, void* stream);
#ifdef __cplusplus
}
#endif
