// Host-only half of the loudness measurement (loudness.h): the K-weighting coefficients of a sample rate and the constants of the chunk
// kernel's scan, in double.  Plain C++17: no HIP header, no device code (cmtts_loudness_coefficients exposes the coefficients to the CPU tests).
//
// Coefficients (cmtts_amd/loudness.py: k_weighting): bilinear transform of the analogue prototypes with K = tan(pi f0 / fs).
//   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; Vh = 10^(G / 20), Vb = Vh^0.4996667741545416;
//              a0 = 1 + K / Q + K^2; b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0; a = [2 (K^2 - 1), 1 - K / Q + K^2] / a0
//   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a as above
// At 48 kHz these are the ITU-R BS.1770-4 table values to all printed digits.
#include <cmath>
#include <cstring>

#include "loudness.h"

namespace {

constexpr double kPi = 3.14159265358979323846;

bool rate_ok(int fs) { return fs >= LD_MIN_RATE && fs <= LD_MAX_RATE && fs % 10 == 0; }

void matmul4(const double* x, const double* y, double* out) {
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += x[i * 4 + k] * y[k * 4 + j];
            t[i * 4 + j] = s;
        }
    memcpy(out, t, sizeof t);
}

}  // namespace

int loudness_coefficients(int fs, double* out10) {
    if (!out10 || !rate_ok(fs)) return -1;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(kPi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out10[0] = (Vh + Vb * K / Q + K * K) / a0;
        out10[1] = 2.0 * (K * K - Vh) / a0;
        out10[2] = (Vh - Vb * K / Q + K * K) / a0;
        out10[3] = 2.0 * (K * K - 1.0) / a0;
        out10[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(kPi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        out10[5] = 1.0;
        out10[6] = -2.0;
        out10[7] = 1.0;
        out10[8] = 2.0 * (K * K - 1.0) / a0;
        out10[9] = (1.0 - K / Q + K * K) / a0;
    }
    return 0;
}

int loudness_plan(int fs, LoudnessPlan* plan) {
    double co[10];
    if (!plan || loudness_coefficients(fs, co) != 0) return -1;
    plan->fs = fs;
    plan->chunk = fs / 10;
    plan->run = ((3 * plan->chunk + LD_THREADS - 1) / LD_THREADS) | 1;          // odd: lanes a run apart fall on different LDS banks
    for (int i = 0; i < 5; ++i) {
        plan->b[i] = (float)co[i];
        plan->c[i] = (float)co[5 + i];
    }
    // one zero-input sample of the cascade in the kernel's own (float) coefficients: u = z1, o = c0 u + w1
    const double a1 = plan->b[3], a2 = plan->b[4], c0 = plan->c[0], c1 = plan->c[1], c2 = plan->c[2], d1 = plan->c[3], d2 = plan->c[4];
    const double A[16] = {-a1, 1, 0, 0, -a2, 0, 0, 0, c1 - d1 * c0, 0, -d1, 1, c2 - d2 * c0, 0, -d2, 0};
    double P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, sq[16];
    memcpy(sq, A, sizeof sq);
    for (int e = plan->run; e; e >>= 1) {          // P = A^run by squaring
        if (e & 1) matmul4(P, sq, P);
        matmul4(sq, sq, sq);
    }
    for (int j = 0; j < LD_SCAN_STEPS; ++j) {
        for (int i = 0; i < 16; ++i) plan->P[j][i] = (float)P[i];
        matmul4(P, P, P);
    }
    return 0;
}
