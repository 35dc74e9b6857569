// ss_resample_host.cpp — the resampler's host arithmetic (include/soundscope_hip.h, "Batch resampler"): the plan rule, the Kaiser-windowed
// sinc table and the reference chain ss_resample_host, which DEFINES what ss_batch_resample's kernels (ss_resample.hip) compute, in
// bits.  No device is needed by anything here.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/soundscope_hip.h"

namespace {

constexpr double kPi = 3.14159265358979323846;

// the modified Bessel function of order 0 by its power series, sum ((x / 2)^k / k!)^2: every term positive, below 1e-17 of the sum
// after fifty of them at the largest beta the plan rule gives (14.5)
double bessel_i0(double x)
{
    const double h = 0.5 * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

bool plan_ok(const ss_resample_plan *p)
{
    return p && p->up && p->down && p->taps >= 4u && !(p->taps & 3u) && (uint64_t)p->up * p->taps <= SS_RESAMPLE_TAPS_MAX;
}

}  // namespace

extern "C" {

int ss_resample_plan_make(uint32_t in_rate, uint32_t out_rate, double attenuation_db, double passband, ss_resample_plan *out)
{
    if (!out || !in_rate || !out_rate || in_rate == out_rate) return SS_ERR_INVALID_ARG;
    const double A = attenuation_db == 0.0 ? 100.0 : attenuation_db;
    const double pb = passband == 0.0 ? 20000.0 / 22050.0 : passband;
    if (!(A >= 40.0 && A <= 140.0) || !(pb >= 0.5 && pb <= 0.99)) return SS_ERR_INVALID_ARG;      // (a NaN fails the comparisons)
    const uint32_t g = gcd_u32(in_rate, out_rate), L = out_rate / g, M = in_rate / g;
    const double ratio = (double)L / (double)M;
    const double fc = 0.5 * (ratio < 1.0 ? ratio : 1.0);
    const double delta = 2.0 * (1.0 - pb) * fc;
    const double beta = 0.1102 * (A - 8.7);
    const double want = std::ceil((A - 7.95) / (14.36 * delta));
    if (!(want * (double)L <= (double)SS_RESAMPLE_TAPS_MAX)) return SS_ERR_UNSUPPORTED;
    uint32_t T = want < 4.0 ? 4u : (uint32_t)want;
    T = (T + 3u) & ~3u;
    if ((uint64_t)L * T > SS_RESAMPLE_TAPS_MAX) return SS_ERR_UNSUPPORTED;
    ss_resample_plan p;
    std::memset(&p, 0, sizeof p);
    p.in_rate = in_rate; p.out_rate = out_rate; p.up = L; p.down = M; p.taps = T; p.reserved = 0;
    p.attenuation_db = A; p.passband = pb; p.beta = beta; p.cutoff = fc;
    *out = p;
    return SS_OK;
}

int ss_resample_taps(const ss_resample_plan *p, float *taps, size_t cap_floats)
{
    if (!plan_ok(p) || !taps || !(p->cutoff > 0.0) || !(p->beta >= 0.0)) return SS_ERR_INVALID_ARG;
    const uint32_t L = p->up, T = p->taps;
    if (cap_floats < (size_t)L * T) return SS_ERR_CAPACITY;
    const bool whole = L >= p->down;                             // 2 fc = 1: the sinc on the integer numerator
    const double two_fc = 2.0 * p->cutoff, i0_beta = bessel_i0(p->beta);
    for (uint32_t ph = 0; ph < L; ph++) {
        double sum = 0.0;
        float *row = taps + (size_t)ph * T;
        for (int pass = 0; pass < 2; pass++) {                   // the row's sum in f64, then every value over it
            for (uint32_t k = 0; k < T; k++) {
                const long long j = ((long long)k - (long long)(T / 2u) + 1) * (long long)L - (long long)ph;
                const double t = (double)j / (double)L;
                double s;
                if (whole) s = j == 0 ? 1.0 : (j % (long long)L == 0 ? 0.0 : std::sin(kPi * t) / (kPi * t));
                else { const double x = two_fc * t; s = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x); }
                const double u = 2.0 * t / (double)T, inside = 1.0 - u * u;
                const double v = two_fc * s * bessel_i0(p->beta * std::sqrt(inside > 0.0 ? inside : 0.0)) / i0_beta;
                if (pass == 0) sum += v; else row[k] = (float)(v / sum);
            }
        }
    }
    return SS_OK;
}

uint64_t ss_resample_length(const ss_resample_plan *p, uint64_t frames_in)
{
    if (!p || !p->up || !p->down) return 0;
    return (frames_in * p->up + p->down - 1u) / p->down;
}

int ss_resample_host(const ss_resample_plan *p, const float *taps, const float *in, uint64_t frames_in, uint32_t channels,
                     uint64_t first_out, uint64_t n_out, float *out)
{
    if (!plan_ok(p) || !taps || !channels || (!in && frames_in) || (!out && n_out)) return SS_ERR_INVALID_ARG;
    const uint64_t length = ss_resample_length(p, frames_in);
    if (first_out > length || n_out > length - first_out) return SS_ERR_INVALID_ARG;
    const uint64_t L = p->up, M = p->down, T = p->taps, C = channels;
    for (uint64_t i = 0; i < n_out; i++) {
        const uint64_t q = (first_out + i) * M, base = q / L;
        const float *row = taps + (size_t)(q % L) * T;
        const long long at = (long long)base - (long long)(T / 2u) + 1;
        // (a tap whose frame lies outside the stream takes its step too, on a zero: the chain stays literal)
        for (uint64_t c = 0; c < C; c++) {
            float acc = 0.0f;
            for (uint64_t k = 0; k < T; k++) {
                const long long f = at + (long long)k;
                const float x = f >= 0 && (uint64_t)f < frames_in ? in[(size_t)f * C + c] : 0.0f;
                acc = fmaf(row[k], x, acc);
            }
            out[(size_t)i * C + c] = acc;
        }
    }
    return SS_OK;
}

}  // extern "C"
