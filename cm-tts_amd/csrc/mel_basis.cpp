// Host-only half of the recorded-speech analysis (mel_analysis.h): the Slaney mel filterbank, the periodic Hann window and the FFT twiddles, in
// double, rounded to float once.  Plain C++17: no HIP header, no device code (cmtts_mel_basis exposes the basis to the CPU tests).
//
// The filterbank (cmtts_amd/analysis.py: mel_basis): the mel scale is linear below 1000 Hz at 200 / 3 Hz per mel and logarithmic above with step
// ln(6.4) / 27; n_mels + 2 corners f[] equally spaced in mel between fmin and fmax; filter i is the triangle rising over [f[i], f[i+1]] and
// falling over [f[i+1], f[i+2]] sampled on linspace(0, fs / 2, n_fft / 2 + 1), scaled by 2 / (f[i+2] - f[i]).
#include <cmath>
#include <vector>

#include "mel_analysis.h"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kFsp = 200.0 / 3.0, kBreakHz = 1000.0, kBreakMel = kBreakHz / kFsp;

double hz_to_mel(double f) { return f >= kBreakHz ? kBreakMel + std::log(f / kBreakHz) / (std::log(6.4) / 27.0) : f / kFsp; }
double mel_to_hz(double m) { return m >= kBreakMel ? kBreakHz * std::exp((std::log(6.4) / 27.0) * (m - kBreakMel)) : kFsp * m; }

// numpy.linspace(a, b, n)[i]
double linspace(double a, double b, int n, int i) { return i == n - 1 ? b : a + i * ((b - a) / (n - 1)); }

}  // namespace

int mel_basis(int fs, int n_fft, int n_mels, double fmin, double fmax, float* out) {
    // an odd n_fft (the GE2E front end's 551, ge2e.hip) has n_fft / 2 + 1 bins on the same linspace(0, fs / 2, bins)
    if (!out || fs < 1 || n_fft < 2 || n_fft > 65536 || n_mels < 1 || n_mels > 1024) return -1;
    if (!(fmin >= 0.0) || !(fmin < fmax) || !(fmax <= fs / 2.0)) return -1;
    const int bins = n_fft / 2 + 1;
    std::vector<double> f(n_mels + 2);
    const double m0 = hz_to_mel(fmin), m1 = hz_to_mel(fmax);
    for (int i = 0; i < n_mels + 2; ++i) f[i] = mel_to_hz(linspace(m0, m1, n_mels + 2, i));
    for (int i = 0; i < n_mels; ++i) {
        const double up = f[i + 1] - f[i], down = f[i + 2] - f[i + 1], norm = 2.0 / (f[i + 2] - f[i]);
        for (int k = 0; k < bins; ++k) {
            const double hz = linspace(0.0, fs / 2.0, bins, k);
            const double lower = -(f[i] - hz) / up, upper = (f[i + 2] - hz) / down;
            const double w = std::fmax(0.0, std::fmin(lower, upper));
            out[(long)i * bins + k] = (float)(w * norm);
        }
    }
    return 0;
}

void mel_window(float* out) {
    for (int u = 0; u < MEL_NFFT; ++u) out[u] = (float)(0.5 - 0.5 * std::cos(2.0 * kPi * u / MEL_NFFT));
}

void mel_twiddles(float* out) {
    for (int k = 0; k < MEL_NFFT / 2; ++k) {
        const double a = -2.0 * kPi * k / MEL_NFFT;
        out[2 * k] = (float)std::cos(a);
        out[2 * k + 1] = (float)std::sin(a);
    }
}

int mel_sparse_rows(const float* basis, float* pack, int32_t* tab) {
    int nnz = 0;
    for (int m = 0; m < MEL_CH; ++m) {
        const float* row = basis + (long)m * MEL_BINS;
        int lo = 0, hi = MEL_BINS;
        while (lo < MEL_BINS && row[lo] == 0.f) ++lo;
        while (hi > lo && row[hi - 1] == 0.f) --hi;
        if (nnz + (hi - lo) > MEL_NNZ_MAX) return -1;
        tab[3 * m] = nnz;
        tab[3 * m + 1] = lo;
        tab[3 * m + 2] = hi - lo;
        for (int k = lo; k < hi; ++k) pack[nnz++] = row[k];      // zeros inside a run (none for a triangle) would be kept: the sum is unchanged
    }
    return nnz;
}
