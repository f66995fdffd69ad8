// Host-only half of the pitch analysis (pitch.h): the geometry, the Hann window and its autocorrelation, the log2 table of the lags and the
// periodised wavelets of the CWT, in double, rounded once.  Plain C++17: no HIP header, no device code.
//
// The CWT tables (cmtts_amd/pitch.py: cwt_table): pycwt multiplies the N-point DFT of the signal by F_j[k] = sqrt(s_j w_1 N) psi^(s_j w_k),
// w_k = 2 pi fftfreq(N, dt)[k], psi^(w) = w^2 exp(-w^2 / 2) / sqrt(Gamma(2.5)), and transforms back.  w_1 N = 2 pi / dt, F_j is real and even
// and F_j[0] = 0, so the product is a circular convolution with h_j[m] = (1 / N) (2 sum_{0 < k < N/2} F_j[k] cos(2 pi k m / N) + F_j[N/2] (-1)^m),
// itself real and even: computed for m <= N / 2 and mirrored.
#include <cmath>
#include <vector>

#include "pitch.h"

namespace {
constexpr double kPi = 3.14159265358979323846;
constexpr double kDt = 0.005, kS0 = 0.01;
}  // namespace

int pitch_geometry(int fs, int hop, double floor_hz, double ceiling_hz, PitchGeometry* g) {
    if (!g || fs < 1 || hop < 1 || hop > PT_MAX_HOP) return -1;
    if (!(floor_hz > 0.0) || !(floor_hz < ceiling_hz) || !(ceiling_hz <= fs / 2.0)) return -1;
    const double w = std::ceil(3.0 * fs / floor_hz);
    if (w > PT_MAX_W) return -1;
    g->fs = fs;
    g->hop = hop;
    g->W = (int)w + ((int)w & 1);
    g->lmin = (int)std::ceil(fs / ceiling_hz);
    g->lmax = (int)std::floor(fs / floor_hz);
    if (g->W > PT_MAX_W || g->lmax + 2 > PT_MAX_LAGS || g->lmin < 1 || g->lmin > g->lmax || g->lmax + 2 > g->W) return -1;
    return 0;
}

void pitch_window(const PitchGeometry& g, float* window, double* rw) {
    std::vector<double> w(g.W);
    for (int i = 0; i < g.W; ++i) {
        w[i] = 0.5 - 0.5 * std::cos(2.0 * kPi * (i + 0.5) / g.W);
        window[i] = (float)w[i];
    }
    double a0 = 0.0;
    for (int tau = 0; tau < g.lmax + 2; ++tau) {
        double a = 0.0;
        for (int i = 0; i + tau < g.W; ++i) a += w[i] * w[i + tau];
        if (tau == 0) a0 = a;
        rw[tau] = a / a0;
    }
}

void pitch_lg(const PitchGeometry& g, double floor_hz, float* lg, float* lg_floor) {
    lg[0] = 0.f;
    for (int tau = 1; tau < g.lmax + 2; ++tau) lg[tau] = (float)std::log2((double)tau);
    *lg_floor = (float)std::log2(g.fs / floor_hz);
}

void pitch_cwt_tables(float* out) {
    const double norm = 1.0 / std::sqrt(std::tgamma(2.5));
    for (int N = PT_CWT_MIN_N; N <= PT_CWT_MAX_N; N *= 2) {
        const int H = N / 2;
        std::vector<double> c(N), F(H + 1), h(H + 1);
        for (int q = 0; q < N; ++q) c[q] = std::cos(2.0 * kPi * q / N);
        for (int j = 0; j < PT_CWT_SCALES; ++j) {
            const double s = kS0 * std::ldexp(1.0, j);
            for (int k = 0; k <= H; ++k) {
                const double sw = s * (2.0 * kPi * k / (N * kDt));
                F[k] = std::sqrt(s * 2.0 * kPi / kDt) * (sw * sw * std::exp(-0.5 * sw * sw) * norm);
            }
            for (int m = 0; m <= H; ++m) {
                double acc = 0.0;
                for (int k = 1; k < H; ++k) acc += F[k] * c[(int)(((long)k * m) & (N - 1))];
                h[m] = (2.0 * acc + ((m & 1) ? -F[H] : F[H])) / N;
            }
            float* dst = out + (long)j * PT_CWT_LD + (N - PT_CWT_MIN_N);
            for (int m = 0; m < N; ++m) dst[m] = (float)h[m <= H ? m : N - m];
        }
    }
}
