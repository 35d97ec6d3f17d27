// design.hpp -- host-side (cold path) filter design and integer bookkeeping for the HIP kernels.
//
// The reference builds its filters on a worker thread by calling liquid-dsp 1.5.0 create() functions
// (DemodulatorWorkerThread.cpp:63-101, ModemAnalog.cpp:21-33, SDRPostThread.cpp:29,406, ModemAM.cpp:9,
// ModemUSB.cpp:8-11).  The GPU kernels need the same coefficient sets as plain arrays, so this file
// computes them on the host with the arithmetic liquid 1.5.0 uses (float where the rounding decides an
// integer such as a filter length or a phase step) and uploads them once per
// (re)configuration.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <complex>
#include <vector>

#include "../../include/csdr_hip.h"

namespace csdr {
namespace design {

constexpr float kPi = 3.14159265358979323846f;

// ---- Kaiser-window prototype design (liquid firdes.c / math.bessel.c / windows.c semantics) ----------------
inline float lngamma_f(float z) {
    // recursion below 10, Stirling-like closed form above (liquid math.gamma.c)
    float shift = 0.0f;
    while (z < 10.0f) { shift += std::log(z); z += 1.0f; }
    float g = 0.5f * (std::log(2.0f * kPi) - std::log(z));
    g += z * (std::log(z + (1.0f / (12.0f * z - 0.1f / z))) - 1.0f);
    return g - shift;
}

inline float bessel_i0_f(float z) {
    if (z == 0.0f) return 1.0f;
    float acc = 0.0f;
    const float lz = std::log(0.5f * z);
    for (unsigned k = 0; k < 32; ++k) acc += std::exp(2.0f * ((float)k * lz - lngamma_f((float)k + 1.0f)));
    return acc;
}

inline float sinc_f(float x) {
    if (std::fabs(x) < 0.01f) return std::cos(kPi * x / 2.0f) * std::cos(kPi * x / 4.0f) * std::cos(kPi * x / 8.0f);
    return std::sin(kPi * x) / (kPi * x);
}

inline float kaiser_beta(float as) {
    as = std::fabs(as);
    if (as > 50.0f) return 0.1102f * (as - 8.7f);
    if (as > 21.0f) return 0.5842f * std::pow(as - 21.0f, 0.4f) + 0.07886f * (as - 21.0f);
    return 0.0f;
}

inline float kaiser_window(unsigned i, unsigned n, float beta) {
    const float t = (float)i - (float)(n - 1) / 2;
    const float r = 2.0f * t / (float)(n - 1);
    return bessel_i0_f(beta * std::sqrt(1 - r * r)) / bessel_i0_f(beta);
}

inline unsigned required_filter_len(float df, float as) { return (unsigned)((as - 7.95f) / (14.26f * df)); }

inline std::vector<float> kaiser_lowpass(unsigned n, float fc, float as) {
    std::vector<float> h(n);
    const float beta = kaiser_beta(as);
    for (unsigned i = 0; i < n; ++i) {
        const float t = (float)i - (float)(n - 1) / 2;
        h[i] = sinc_f(2.0f * fc * t) * kaiser_window(i, n, beta);
    }
    return h;
}

// ---- half-band filters ---------------------------------------------------------------------------------------
// liquid 1.5.0 designs resamp2's prototype with an iterative equiripple optimiser whose result is not a closed
// form.  CubicSDR creates every msresamp with As = 60 dB (DemodulatorWorkerThread.cpp:100, ModemAnalog.cpp:25,
// SpectrumVisualProcessor.cpp:361), msresamp2 adds 5 dB, and the stage rule below only ever yields m = 10, 5, 3.
// Those three coefficient sets are design constants of the reference's DSP library, tabulated here (first half of
// the symmetric odd-tap branch; the centre tap acts as a pure delay).  Other (m, As) fall back to a Kaiser
// half-band and are reported as not parity-pinned.
inline bool halfband_branch(unsigned m, float as, std::vector<float> &h1, bool *pinned = nullptr) {
    static const float t3[3] = {0x1.31fb88p-6f, -0x1.d5fe0ep-4f, 0x1.31556cp-1f};
    static const float t5[5] = {0x1.4ae43ap-8f, -0x1.679e46p-6f, 0x1.084878p-4f, -0x1.57458ap-3f, 0x1.3da7d4p-1f};
    static const float t10[10] = {-0x1.7604f2p-10f, 0x1.caf71ap-9f, -0x1.e992e0p-8f, 0x1.cc3ab4p-7f, -0x1.8f23dcp-6f,
                                  0x1.495b22p-5f,   -0x1.0a5864p-4f, 0x1.b87790p-4f, -0x1.992bc8p-3f, 0x1.43c83ep-1f};
    const float *t = nullptr;
    if (std::fabs(as - 65.0f) < 1e-3f) t = (m == 3) ? t3 : (m == 5) ? t5 : (m == 10) ? t10 : nullptr;
    h1.assign(2 * m, 0.0f);
    if (pinned) *pinned = (t != nullptr);
    if (t) {
        for (unsigned i = 0; i < m; ++i) h1[i] = h1[2 * m - 1 - i] = t[i];
        return true;
    }
    const unsigned n = 4 * m + 1;
    const float beta = kaiser_beta(as);
    for (unsigned j = 0, i = 1; i < n; i += 2, ++j) {
        const float tt = (float)i - (float)(n - 1) / 2.0f;
        h1[j] = sinc_f(tt / 2.0f) * kaiser_window(i, n, beta);
    }
    return true;
}

// ---- multi-stage resampler plan (msresamp + msresamp2 + resamp of liquid 1.5.0) ----------------------------
struct MsresampPlan {
    bool interp = false;        // rate > 1
    unsigned S = 0;             // number of half-band stages
    float rate_arb = 1.0f;      // arbitrary stage rate in [0.5, 1) (decim) or (1, 2] (interp)
    uint32_t step = 0;          // round(2^24 / rate_arb)
    std::vector<unsigned> m;    // per design index (index 0 = lowest-rate stage)
    std::vector<std::vector<float>> h1;  // per design index: 2m symmetric taps of the filtered branch
    std::vector<float> arms;    // [256][14] arbitrary-resampler polyphase bank, oldest-sample-first
    bool pinned = true;         // false if a non-tabulated half-band was needed
    static constexpr unsigned kArms = 256, kArmTaps = 14;
};

inline MsresampPlan plan_msresamp(float rate, float as) {
    MsresampPlan p;
    p.interp = rate > 1.0f;
    p.rate_arb = rate;
    if (p.interp) while (p.rate_arb > 2.0f) { ++p.S; p.rate_arb *= 0.5f; }
    else          while (p.rate_arb < 0.5f) { ++p.S; p.rate_arb *= 2.0f; }
    // half-band stages: msresamp2_create(type, S, fc = 0.4, f0 = 0, As)
    float fc = 0.4f;
    const float as2 = as + 5.0f;
    for (unsigned i = 0; i < p.S; ++i) {
        fc = (i == 1) ? (0.5f - fc) * 0.5f : 0.5f * fc;
        const float ft = 2 * (0.25f - fc);
        const unsigned hl = required_filter_len(ft, as2);
        unsigned mm = (unsigned)std::ceil((float)(hl - 1) / 4.0f);
        if (mm < 3) mm = 3;
        std::vector<float> h;
        bool pin = true;
        halfband_branch(mm, as2, h, &pin);
        p.pinned = p.pinned && pin;
        p.m.push_back(mm);
        p.h1.push_back(h);
    }
    // arbitrary stage: resamp_create(rate_arb, m = 7, fc = min(0.515 rate_arb, 0.49), As, npfb = 256)
    float fca = 0.515f * p.rate_arb;
    if (fca > 0.49f) fca = 0.49f;
    p.step = (uint32_t)std::round((float)(1u << 24) / p.rate_arb);
    const unsigned npfb = MsresampPlan::kArms, sub = MsresampPlan::kArmTaps, n = sub * npfb + 1;
    std::vector<float> hf = kaiser_lowpass(n, fca / (float)npfb, as);
    float gain = 0.0f;
    for (float v : hf) gain += v;
    gain = (float)npfb / gain;
    p.arms.resize((size_t)npfb * sub);
    for (unsigned a = 0; a < npfb; ++a)
        for (unsigned k = 0; k < sub; ++k) p.arms[a * sub + (sub - 1 - k)] = hf[a + k * npfb] * gain;
    return p;
}

// number of arbitrary-stage outputs produced while consuming K inputs starting at 24-bit phase `phase`,
// and the phase afterwards (closed form of the while-loop in resamp_execute)
inline uint64_t resamp_count(uint64_t K, uint32_t phase, uint32_t step, uint32_t *phase_after) {
    const uint64_t lim = K << 24;
    uint64_t J = 0;
    if (lim > phase) J = (lim - phase + step - 1) / step;
    if (phase_after) *phase_after = (uint32_t)((uint64_t)phase + J * step - lim);
    return J;
}

// ---- NCO frequency word (nco_crcf_set_frequency of liquid 1.5.0: float -> uint32) ---------
inline uint32_t nco_phase_word(float theta) {
    const float p = (float)((double)theta * 0.159154943091895);
    float frac = p - (float)((long)p);
    if (frac < 0.0f) frac += 1.0f;
    return (uint32_t)(int64_t)(frac * 4294967296.0f);
}
inline std::vector<float> nco_sine_table() {
    std::vector<float> t(1024);
    // the argument is formed in float, its sine correctly rounded (the reference binary's table bit for bit; glibc's sinf differs in 15 entries)
    for (unsigned i = 0; i < 1024; ++i) t[i] = (float)std::sin((double)(2.0f * kPi * (float)i / 1024.0f));
    return t;
}

// ---- polyphase analysis channelizer prototype (firpfbch_crcf_create_kaiser(ANALYZER, M, m, As)) ------------
// returns taps[c][n] (c = commutator position 0..M-1, n = 0..2m-1 frames back) such that
//   X_t[c] = sum_n taps[c][n] * x[(t - n) * M + c]        and    y_t[k] = sum_c X_t[c] exp(-j 2 pi k c / M)
inline std::vector<float> channelizer_taps(unsigned M, unsigned m, float as) {
    const unsigned p = 2 * m, hl = 2 * M * m + 1;
    std::vector<float> h = kaiser_lowpass(hl, 0.5f / (float)M, as);
    std::vector<float> t((size_t)M * p);
    for (unsigned c = 0; c < M; ++c)
        for (unsigned n = 0; n < p; ++n) t[(size_t)c * p + n] = h[(M - 1 - c) + n * M];
    return t;
}

// ---- 2x oversampled polyphase analysis channelizer (firpfbch2_crcf_create_kaiser(ANALYZER, M, m, As)) --------
// liquid 1.5.0 firpfbch2: prototype Kaiser low-pass of 2 M m + 1 taps with cut-off 1/M (twice the analyzer bandwidth of
// firpfbch), scaled to sum M; every execute() takes M/2 new samples and applies the first 2 M m taps, an M-point inverse
// DFT and a 1/M gain, with the branch order rotating by M/2 on alternate calls.  Written in the commutator form of
// channelizer_taps (pinned against the reference DLL's impulse responses to 1e-7):
//   X_t[c] = sum_n taps[c][n] x[(t - 1) M/2 + c - n M]
//   y_t[k] = post[t & 1][k] sum_c X_t[c] exp(-j 2 pi k c / M),   post[p][k] = (p ? (-1)^k : 1) exp(-j 2 pi k / M) / M
inline std::vector<float> channelizer2_taps(unsigned M, unsigned m, float as) {
    const unsigned p = 2 * m, hl = 2 * M * m + 1;
    std::vector<float> h = kaiser_lowpass(hl, 1.0f / (float)M, as);
    float sum = 0.0f;
    for (float v : h) sum += v;
    for (float &v : h) v = v * (float)M / sum;
    std::vector<float> t((size_t)M * p);
    for (unsigned c = 0; c < M; ++c)
        for (unsigned n = 0; n < p; ++n) t[(size_t)c * p + n] = h[(M - 1 - c) + n * M];
    return t;
}
// post[2][M] as (re, im) pairs
inline std::vector<float> channelizer2_post(unsigned M) {
    std::vector<float> t((size_t)4 * M);
    for (unsigned par = 0; par < 2; ++par)
        for (unsigned k = 0; k < M; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)M;
            const double s = (par && (k & 1)) ? -1.0 : 1.0;
            t[2 * ((size_t)par * M + k)] = (float)(s * std::cos(a) / (double)M);
            t[2 * ((size_t)par * M + k) + 1] = (float)(s * std::sin(a) / (double)M);
        }
    return t;
}

// ---- AM DC-blocking FIR (firfilt_rrrf_create_dc_blocker(m, As) -> liquid_firdes_notch(m, 0, As)) -----------
inline std::vector<float> dc_notch_taps(unsigned m, float as) {
    const unsigned n = 2 * m + 1;
    const float beta = kaiser_beta(as);
    std::vector<float> h(n);
    float scale = 0.0f;
    for (unsigned i = 0; i < n; ++i) {
        const float p = -1.0f;  // -cos(2 pi f0 (i - m)) with f0 = 0
        h[i] = p * kaiser_window(i, n, beta);
        scale += h[i] * p;
    }
    for (float &v : h) v /= scale;
    h[m] += 1.0f;
    return h;
}

// ---- SSB: Butterworth low-pass as second-order sections (iirfilt_crcf_create_lowpass(order, fc)) -----------
struct Sos { float b[3]; float a[3]; };
inline std::vector<Sos> butter_lowpass_sos(unsigned order, float fc) {
    const unsigned r = order % 2, L = (order - r) / 2;
    const float mm = 1.0f / std::tan(kPi * fc);
    std::vector<Sos> out;
    double gr = 1.0, gi = 0.0;
    std::vector<double> a1, a2;
    for (unsigned i = 0; i < L; ++i) {
        const float th = (float)(2 * (i + 1) + order - 1) * kPi / (float)(2 * order);
        double pr = std::cos(th) / mm, pi = std::sin(th) / mm;
        // digital pole pd = (1 + p) / (1 - p), and its conjugate
        double dr = 1.0 - pr, di = -pi, nr = 1.0 + pr, ni = pi, den = dr * dr + di * di;
        double qr = (nr * dr + ni * di) / den, qi = (ni * dr - nr * di) / den;
        // gain *= (1 - pd)(1 - conj pd) / 4
        double f = ((1.0 - qr) * (1.0 - qr) + qi * qi) / 4.0;
        gr *= f;
        a1.push_back(-2.0 * qr);
        a2.push_back(qr * qr + qi * qi);
    }
    double real_pole = 0.0;
    if (r) { double pr = -1.0 / mm; real_pole = (1.0 + pr) / (1.0 - pr); gr *= (1.0 - real_pole) / 2.0; }
    (void)gi;
    const float kg = std::pow((float)gr, 1.0f / (float)(L + r));
    // the reference orders its sections by ascending a2 (pinned by tests against the reference binary)
    for (unsigned i = 0; i < L; ++i)
        for (unsigned j = i + 1; j < L; ++j)
            if (a2[j] < a2[i]) { std::swap(a2[i], a2[j]); std::swap(a1[i], a1[j]); }
    for (unsigned i = 0; i < L; ++i) out.push_back(Sos{{kg, 2.0f * kg, kg}, {1.0f, (float)a1[i], (float)a2[i]}});
    if (r) out.push_back(Sos{{kg, kg, 0.0f}, {1.0f, (float)(-real_pole), 0.0f}});
    return out;
}

// impulse response of a cascade of second-order sections (direct form II, as iirfilt_crcf_execute runs them), n samples, in
// double: the SSB low-pass has poles of radius <= 0.77, so its response is below 1e-14 of the peak after 128 samples and the
// recursive filter IS (to far below float32 resolution) the FIR filter with these taps -- which runs in parallel
inline std::vector<float> sos_impulse_response(const std::vector<Sos> &sos, unsigned n) {
    std::vector<double> v1(sos.size(), 0.0), v2(sos.size(), 0.0);
    std::vector<float> g(n);
    for (unsigned i = 0; i < n; ++i) {
        double t = i == 0 ? 1.0 : 0.0;
        for (size_t q = 0; q < sos.size(); ++q) {
            const double v0 = t - (double)sos[q].a[1] * v1[q] - (double)sos[q].a[2] * v2[q];
            t = (double)sos[q].b[0] * v0 + (double)sos[q].b[1] * v1[q] + (double)sos[q].b[2] * v2[q];
            v2[q] = v1[q]; v1[q] = v0;
        }
        g[i] = (float)t;
    }
    return g;
}

// ---- FM stereo: 19 kHz pilot band-pass (iirfilt_crcf_create_prototype(CHEBY2, BANDPASS, SOS, 5, fc, f0, 1, 60), ModemFMStereo.cpp:128-139) ----
// liquid_iirdes of liquid 1.5.0 restated with its single-precision data flow (cheby2_azpkf -> bilinear_zpkf -> iirdes_dzpk_lp2bp ->
// iirdes_dzpk2sosf): the pole radii are ~0.998, so the pass-band phase moves by 1e-4 rad per unit in the last place of a feedback
// coefficient, and only the same roundings give the same filter.  Complex quotients of floats are formed the plain way
// ((a conj b) / |b|^2), the bilinear map runs in double (its "1.0" literals promote the operands); pinned bit-for-bit against the
// reference binary on 400 sample rates (feedback taps always; 3 of 400 feed-forward taps differ by one unit in the last place).
inline std::vector<Sos> cheby2_bandpass_sos(unsigned n, float fc, float f0, float as) {
    typedef std::complex<float> cf;
    typedef std::complex<double> cd;
    const double pi = 3.14159265358979323846;
    auto qf = [](cf a, cf b) { const float d = b.real() * b.real() + b.imag() * b.imag();
                               return cf((a.real() * b.real() + a.imag() * b.imag()) / d, (a.imag() * b.real() - a.real() * b.imag()) / d); };
    auto qd = [](cd a, cd b) { const double d = b.real() * b.real() + b.imag() * b.imag();
                               return cd((a.real() * b.real() + a.imag() * b.imag()) / d, (a.imag() * b.real() - a.real() * b.imag()) / d); };
    const unsigned r = n % 2, L = (n - r) / 2;
    const float es = std::pow(10.0f, -as / 20.0f);
    const float t0 = (float)std::sqrt(1.0 + 1.0 / ((double)es * (double)es));
    const float tp = std::pow((float)((double)t0 + 1.0 / (double)es), (float)(1.0 / (double)(float)n));
    const float tm = std::pow((float)((double)t0 - 1.0 / (double)es), (float)(1.0 / (double)(float)n));
    const float eb = (float)(0.5 * ((double)tp + (double)tm)), ea = (float)(0.5 * ((double)tp - (double)tm));
    std::vector<cf> pa, za;
    for (unsigned i = 0; i < L; ++i) {
        const float th = (float)((double)(float)(2 * (i + 1) + n - 1) * pi / (double)(float)(2 * n));
        pa.push_back(qf(cf(1.0f, 0.f), cf(ea * std::cos(th), -eb * std::sin(th))));
        pa.push_back(qf(cf(1.0f, 0.f), cf(ea * std::cos(th), eb * std::sin(th))));
    }
    if (r) pa.push_back(cf(-1.0f / ea, 0.f));
    for (unsigned i = 0; i < L; ++i) {
        const float th = (float)(0.5 * pi * (double)(2 * (i + 1) - 1) / (double)(float)n);
        za.push_back(qf(cf(-1.0f, 0.f), cf(0.f, std::cos(th))));
        za.push_back(qf(cf(1.0f, 0.f), cf(0.f, std::cos(th))));
    }
    const float m = std::fabs((std::cos((float)(2 * pi * (double)fc)) - std::cos((float)(2 * pi * (double)f0))) / std::sin((float)(2 * pi * (double)fc)));
    std::vector<cf> zd(n), pd(n);
    cf G(1.0f, 0.f);
    for (unsigned i = 0; i < n; ++i) {
        if (i < 2 * L) { const cf zm = za[i] * m; zd[i] = (cf)qd(cd(1.0) + (cd)zm, cd(1.0) - (cd)zm); } else zd[i] = cf(-1.0f, 0.f);
        const cf pm = pa[i] * m;
        pd[i] = (cf)qd(cd(1.0) + (cd)pm, cd(1.0) - (cd)pm);
        G = (cf)((cd)G * qd(cd(1.0) - (cd)pd[i], cd(1.0) - (cd)zd[i]));
    }
    const float c0 = std::cos((float)(2 * pi * (double)f0));
    auto lp2bp = [&](const std::vector<cf> &v) {
        std::vector<cf> o;
        for (const cf &z : v) {
            const cf t = cf(1.0f) + z, sq = std::sqrt(c0 * c0 * t * t - 4.0f * z);
            o.push_back(0.5f * (c0 * t + sq));
            o.push_back(0.5f * (c0 * t - sq));
        }
        return o;
    };
    // liquid_cplxpair: conjugate pairs (negative imaginary part first) by ascending real part, then the purely real values
    auto pairup = [](std::vector<cf> v) {
        const float tol = 1e-6f;
        const size_t N = v.size();
        std::vector<bool> used(N, false);
        std::vector<cf> o;
        for (size_t i = 0; i < N; ++i) {
            if (used[i] || std::fabs(v[i].imag()) < tol) continue;
            for (size_t j = 0; j < N; ++j) {
                if (j == i || used[j] || std::fabs(v[j].imag()) < tol) continue;
                if (std::fabs(v[i].imag() + v[j].imag()) < tol && std::fabs(v[i].real() - v[j].real()) < tol) {
                    o.push_back(v[i]); o.push_back(v[j]); used[i] = used[j] = true;
                    break;
                }
            }
        }
        const size_t np = o.size() / 2;
        for (size_t i = 0; i < N; ++i) if (!used[i]) o.push_back(v[i]);
        for (size_t i = 0; i < np; ++i) if (o[2 * i].imag() > 0) std::swap(o[2 * i], o[2 * i + 1]);
        for (size_t i = 0; i < np; ++i)
            for (size_t j = i + 1; j < np; ++j)
                if (o[2 * j].real() < o[2 * i].real()) { std::swap(o[2 * i], o[2 * j]); std::swap(o[2 * i + 1], o[2 * j + 1]); }
        for (size_t i = 2 * np; i < N; ++i)
            for (size_t j = i + 1; j < N; ++j)
                if (o[j].real() < o[i].real()) std::swap(o[i], o[j]);
        return o;
    };
    const std::vector<cf> zp = pairup(lp2bp(zd)), pp = pairup(lp2bp(pd));
    const float kg = std::pow(G.real(), 1.0f / (float)n);
    std::vector<Sos> out;
    for (unsigned i = 0; i < n; ++i) {
        const cf p0 = -pp[2 * i], p1 = -pp[2 * i + 1], z0 = -zp[2 * i], z1 = -zp[2 * i + 1];
        Sos q;
        q.a[0] = 1.0f; q.a[1] = (p0 + p1).real(); q.a[2] = (p0 * p1).real();
        q.b[0] = kg; q.b[1] = (z0 + z1).real() * kg; q.b[2] = (z0 * z1).real() * kg;
        out.push_back(q);
    }
    return out;
}
inline std::vector<Sos> fms_pilot_sos(int64_t sample_rate) {          // ModemFMStereo.cpp:128-139
    float bw = (float)sample_rate;
    if (bw < 100000.0f) bw = 100000.0f;
    return cheby2_bandpass_sos(5, (float)19500 / bw, (float)19000 / bw, 60.0f);
}

// ---- FM stereo: output filter of one channel = de-emphasis (iirfilt_rrrf, one pole: ModemFMStereo.cpp:147-159) followed by the
// 16 kHz Kaiser low-pass (firfilt_rrrf, :107-126), as ONE impulse response (both are LTI and start from rest).  The pole of the
// de-emphasis is at most 0.9 in magnitude at the rates the reference runs (75 us at 96 kHz: -0.87), so its response is cut where
// it falls below 1e-10; demph_us == 0 leaves the low-pass alone.
inline std::vector<float> fms_output_fir(int audio_rate, int demph_us, unsigned max_taps) {
    const float as = 60.0f;
    float fcut = 16000.0f / (float)audio_rate;
    const float ft = 1000.0f / (float)audio_rate;
    if (fcut < 0) fcut = 0;
    if (fcut > 0.5f) fcut = 0.5f;
    const unsigned h_len = required_filter_len(ft, as);
    const std::vector<float> h = kaiser_lowpass(h_len, fcut, as);
    if (!demph_us) return h.size() <= max_taps ? h : std::vector<float>();
    const double f = 1.0 / (2.0 * M_PI * (double)demph_us * 1e-6);
    double t = 1.0 / (2.0 * M_PI * f);
    t = 1.0 / (2.0 * (double)audio_rate * std::tan(1.0 / (2.0 * (double)audio_rate * t)));
    const double tb = 1.0 + 2.0 * t * (double)audio_rate;
    const float b0 = (float)(1.0 / tb), b1 = (float)(1.0 / tb), a1 = (float)((1.0 - 2.0 * t * (double)audio_rate) / tb);
    std::vector<double> dm;
    double v1 = 0.0;
    for (unsigned i = 0; i < 4096; ++i) {                 // direct form II: v0 = x - a1 v1;  y = b0 v0 + b1 v1
        const double v0 = (i == 0 ? 1.0 : 0.0) - (double)a1 * v1;
        dm.push_back((double)b0 * v0 + (double)b1 * v1);
        v1 = v0;
        if (i > 8 && std::fabs(v0) < 1e-10) break;
    }
    if (h.size() + dm.size() - 1 > max_taps) return std::vector<float>();
    std::vector<double> g(h.size() + dm.size() - 1, 0.0);
    for (size_t i = 0; i < h.size(); ++i)
        for (size_t k = 0; k < dm.size(); ++k) g[i + k] += (double)h[i] * dm[k];
    return std::vector<float>(g.begin(), g.end());
}

// ---- SSB: Hilbert transformer taps (firhilbf_create(m, As)); h[n] for odd delays n = 1, 3, .., 4m-1 ---------
// y_q[k] = sum_{n odd} hq[(n-1)/2] * imag(x[k - n]),  y_i[k] = real(x[k - 2m])
inline std::vector<float> hilbert_taps(unsigned m, float as) {
    const unsigned n = 4 * m + 1;
    std::vector<float> h = kaiser_lowpass(n, 0.25f, std::fabs(as));
    std::vector<float> hq;
    for (unsigned i = 1; i < n; i += 2) {
        const float t = (float)i - (float)(n - 1) / 2.0f;
        hq.push_back(h[i] * std::sin(0.5f * kPi * t));
    }
    return hq;
}

// ---- GMSK (ModemGMSK.cpp: gmskdem_create(k, m, BT)): the transmit pulse and the receive filter, h_len = 2 k m + 1 taps each ---------------
// liquid_firdes_gmsktx: the Gaussian-filtered rectangle of one symbol, Q(2 pi BT (t - 1/2) / sqrt(ln 2)) - Q(2 pi BT (t + 1/2) / sqrt(ln 2)) at
// t = i / k - m, scaled to integrate to pi / 2 per symbol, times k.  liquid_firdes_gmskrx: the ratio of the spectra of a Kaiser Nyquist prototype
// (cut-off 1 / 2k, transition BT / k, stop-band from its length) and of that pulse, each lifted by its minimum plus 1e-3, times a Kaiser
// low-pass (cut-off (0.7 + 0.1 BT) / k, 60 dB) normalised to its DC value, back in time and scaled by k^2 / (k h_len).  That ratio is
// ill-conditioned where both spectra lie near their minima -- float32 steps move the taps by up to a few 1e-3 of the peak (14 % in liquid's own
// float design at k 512, m 8, BT 0.1) -- so everything here is evaluated in double, the h_len-point (odd) DFTs by Bluestein's method over a
// power-of-two FFT, and only the taps are rounded to float.
inline double q_function(double z) { return 0.5 * std::erfc(z * 0.70710678118654752440); }

inline double bessel_i0(double z) {          // sum ((z / 2)^k / k!)^2 to double precision
    const double q = 0.25 * z * z;
    double t = 1.0, acc = 1.0;
    for (int k = 1; k < 500 && t > 1e-17 * acc; ++k) { t *= q / ((double)k * k); acc += t; }
    return acc;
}

// the stop-band attenuation whose Kaiser length estimate reaches n taps at transition width df (bisection over (0.01, 200) dB, 20 steps)
inline double required_filter_as(double df, unsigned n) {
    double as0 = 0.01, as1 = 200.0, as = 0.0;
    for (int i = 0; i < 20; ++i) {
        as = 0.5 * (as1 + as0);
        if ((double)(unsigned)((as - 7.95) / (14.26 * df)) < (double)n) as0 = as;
        else as1 = as;
    }
    return as;
}

// the Kaiser-windowed sinc low-pass of liquid_firdes_kaiser in double
inline std::vector<double> kaiser_lowpass_d(unsigned n, double fc, double as) {
    as = std::fabs(as);
    const double beta = as > 50.0 ? 0.1102 * (as - 8.7) : as > 21.0 ? 0.5842 * std::pow(as - 21.0, 0.4) + 0.07886 * (as - 21.0) : 0.0;
    const double i0b = bessel_i0(beta);
    std::vector<double> h(n);
    for (unsigned i = 0; i < n; ++i) {
        const double t = (double)i - (double)(n - 1) / 2.0, r = 2.0 * t / (double)(n - 1), x = 2.0 * fc * t;
        const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        h[i] = sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    }
    return h;
}

// in-place radix-2 forward transform of a power-of-two length; tw: exp(-2 pi i j / n), j < n / 2
inline void fft_pow2(std::vector<std::complex<double>> &a, const std::vector<std::complex<double>> &tw) {
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const size_t h = len / 2, step = n / len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < h; ++k) {
                const std::complex<double> u = a[i + k], v = a[i + k + h] * tw[k * step];
                a[i + k] = u + v; a[i + k + h] = u - v;
            }
    }
}

// n-point DFTs of any length in double: Bluestein's chirp convolution over a power-of-two transform (the chirp's transform made once)
struct DftAny {
    size_t n, L;
    std::vector<std::complex<double>> chirp, B, tw;
    explicit DftAny(size_t n_) : n(n_), L(1) {
        while (L < 2 * n - 1) L <<= 1;
        tw.resize(L / 2);
        for (size_t j = 0; j < L / 2; ++j) tw[j] = std::polar(1.0, -2.0 * M_PI * (double)j / (double)L);
        chirp.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const uint64_t i2 = ((uint64_t)i * i) % (2 * (uint64_t)n);     // exp(-i pi i^2 / n), the square reduced exactly
            chirp[i] = std::polar(1.0, -M_PI * (double)i2 / (double)n);
        }
        B.assign(L, 0.0);
        B[0] = std::conj(chirp[0]);
        for (size_t i = 1; i < n; ++i) B[i] = B[L - i] = std::conj(chirp[i]);
        fft_pow2(B, tw);
    }
    // sign -1: forward, +1: backward (unnormalised)
    std::vector<std::complex<double>> run(const std::vector<std::complex<double>> &x, int sign) const {
        std::vector<std::complex<double>> a(L);
        for (size_t i = 0; i < n; ++i) a[i] = (sign < 0 ? x[i] : std::conj(x[i])) * chirp[i];
        fft_pow2(a, tw);
        for (size_t i = 0; i < L; ++i) a[i] = std::conj(a[i] * B[i]);         // the inverse transform as the conjugate of a forward one
        fft_pow2(a, tw);
        std::vector<std::complex<double>> y(n);
        for (size_t i = 0; i < n; ++i) {
            const std::complex<double> v = std::conj(a[i]) / (double)L * chirp[i];
            y[i] = sign < 0 ? v : std::conj(v);
        }
        return y;
    }
};

inline std::vector<double> gmsk_tx_taps_d(unsigned k, unsigned m, double bt) {
    const unsigned n = 2 * k * m + 1;
    std::vector<double> h(n);
    const double c0 = 1.0 / std::sqrt(std::log(2.0));
    double e = 0.0;
    for (unsigned i = 0; i < n; ++i) {
        const double t = (double)i / (double)k - (double)m;
        h[i] = q_function(2 * M_PI * bt * (t - 0.5) * c0) - q_function(2 * M_PI * bt * (t + 0.5) * c0);
        e += h[i];
    }
    for (unsigned i = 0; i < n; ++i) h[i] *= M_PI / (2.0 * e) * (double)k;
    return h;
}

inline std::vector<float> gmsk_tx_taps(unsigned k, unsigned m, float bt) {
    const std::vector<double> h = gmsk_tx_taps_d(k, m, bt);
    return std::vector<float>(h.begin(), h.end());
}

inline std::vector<float> gmsk_rx_taps(unsigned k, unsigned m, float bt_f) {
    const unsigned n = 2 * k * m + 1, km = k * m;
    const double bt = bt_f;
    const std::vector<double> ht = gmsk_tx_taps_d(k, m, bt);
    const std::vector<double> hp = kaiser_lowpass_d(n, 0.5 / k, required_filter_as(bt / k, n));    // the Nyquist prototype
    const std::vector<double> gp = kaiser_lowpass_d(n, (0.7 + 0.1 * bt) / k, 60.0);                 // the stop-band gain
    std::vector<std::complex<double>> a(n), b(n), c(n);
    for (unsigned i = 0; i < n; ++i) {              // centred on index 0: zero phase, real spectra
        const unsigned j = (i + km) % n;
        a[i] = hp[j]; b[i] = gp[j]; c[i] = ht[j];
    }
    const DftAny dft(n);
    const auto Hp = dft.run(a, -1), Gp = dft.run(b, -1), Ht = dft.run(c, -1);
    double hp_min = 0, gp_min = 0, ht_min = 0;
    for (unsigned i = 0; i < n; ++i) {
        if (i == 0 || Ht[i].real() < ht_min) ht_min = Ht[i].real();
        if (i == 0 || Hp[i].real() < hp_min) hp_min = Hp[i].real();
        if (i == 0 || Gp[i].real() < gp_min) gp_min = Gp[i].real();
    }
    const double delta = 1e-3;
    std::vector<std::complex<double>> H(n);
    for (unsigned i = 0; i < n; ++i)
        H[i] = (Hp[i].real() - hp_min + delta) / (Ht[i].real() - ht_min + delta) * ((Gp[i].real() - gp_min) / Gp[0].real());
    const auto hh = dft.run(H, +1);
    std::vector<float> h(n);
    for (unsigned i = 0; i < n; ++i) h[i] = (float)(hh[(i + km + 1) % n].real() / (double)(k * n) * (double)k * (double)k);
    return h;
}

// ---- the ring description of an APSK constellation from its points (liquid's modemcf APSK objects: concentric rings of evenly spaced points,
// a slicer on |x| midway between neighbouring rings, a symbol map) -- csdr_design_rings, include/csdr_hip.h.  No liquid table enters: the caller
// supplies what modemcf_modulate returns.
struct RingPlan {
    int n_rings = 0;
    int size[8] = {0};
    float radius[8] = {0}, phase[8] = {0}, slicer[8] = {0};
    unsigned char map[256] = {0};          // symbol -> ring-ordered index
};
// false: not 2^k points in 2 .. 256, more than 8 rings, duplicate points, or rings that are not concentric and evenly spaced
inline bool design_rings(const float *pts, int n, RingPlan *out) {
    if (!pts || n < 2 || n > 256 || (n & (n - 1))) return false;
    constexpr double kTwoPi = 6.28318530717958647692, kRadTol = 1e-4, kArgTol = 1e-4;
    std::vector<double> rad((size_t)n);
    std::vector<int> order((size_t)n);
    double rmax = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(pts[2 * i]) || !std::isfinite(pts[2 * i + 1])) return false;
        rad[i] = std::hypot((double)pts[2 * i], (double)pts[2 * i + 1]);
        rmax = std::max(rmax, rad[i]);
        order[i] = i;
    }
    if (!(rmax > 0.0)) return false;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return rad[a] < rad[b]; });
    RingPlan r;
    int base = 0;
    for (int a = 0; a < n;) {
        int e = a + 1;
        while (e < n && rad[order[e]] - rad[order[a]] <= kRadTol * rmax) ++e;
        if (r.n_rings == 8) return false;
        const int l = r.n_rings++, p = e - a;
        double sum = 0.0;
        for (int q = a; q < e; ++q) sum += rad[order[q]];
        r.size[l] = p;
        r.radius[l] = (float)(sum / p);
        if (sum / p <= kRadTol * rmax) {          // the centre: one point, phase 0
            if (p != 1) return false;
            r.phase[l] = 0.0f;
            r.map[order[a]] = (unsigned char)base;
        } else {
            std::vector<double> arg((size_t)p);
            double ph = kTwoPi;
            for (int q = 0; q < p; ++q) {
                const int i = order[a + q];
                double t = std::atan2((double)pts[2 * i + 1], (double)pts[2 * i]);
                if (t < 0.0) t = t > -1e-6 ? 0.0 : t + kTwoPi;
                arg[q] = t;
                ph = std::min(ph, t);
            }
            const double step = kTwoPi / p;
            bool seen[256] = {false};
            for (int q = 0; q < p; ++q) {
                const double u = (arg[q] - ph) / step;
                const long j = std::lround(u);
                if (std::fabs(u - (double)j) * step > kArgTol) return false;
                const int jj = (int)(j % p);
                if (seen[jj]) return false;
                seen[jj] = true;
                r.map[order[a + q]] = (unsigned char)(base + jj);
            }
            r.phase[l] = (float)ph;
        }
        base += p;
        a = e;
    }
    for (int l = 0; l + 1 < r.n_rings; ++l) r.slicer[l] = 0.5f * (r.radius[l] + r.radius[l + 1]);
    *out = r;
    return true;
}

// ---- the waterfall's colour gradient (src/util/Gradient.cpp:37-85, Gradient::generate(len)) ------------------
// n colour stops (r, g, b interleaved) -> len entries per channel: n - 1 chunks of len / (n - 1) entries, the last one longer by the remainder; entry
// i of a chunk is c1 + (c2 - c1) * ((float)i / (float)chunk) with every operation rounded on its own in float, clamped to [0, 1].
// false: fewer than 2 stops or more than len + 1 (the reference divides by a chunk size of 0 there), or a null pointer.
inline bool gradient(const float *stops, int n, int len, float *r, float *g, float *b) {
    if (!stops || !r || !g || !b || len < 1 || n < 2 || n > len + 1) return false;
    size_t chunk = (size_t)len / (size_t)(n - 1), p = 0;
    float *out[3] = {r, g, b};
    for (size_t j = 0, jmax = (size_t)n - 1; j < jmax; ++j) {
        if (chunk * jmax < (size_t)len && j == jmax - 1) chunk += (size_t)len - chunk * jmax;
        for (size_t i = 0; i < chunk; ++i, ++p) {
            const float idx = (float)i / (float)chunk;
            for (int k = 0; k < 3; ++k) {
                const float c1 = stops[3 * j + k], c2 = stops[3 * (j + 1) + k];
                volatile float d = c2 - c1;              // (volatile: each step is stored as a float, whatever the compiler's contraction rule)
                volatile float m = d * idx;
                float c = c1 + m;
                if (c < 0.0f) c = 0.0f;
                if (c > 1.0f) c = 1.0f;
                out[k][p] = c;
            }
        }
    }
    return true;
}
// the 256-entry RGBA8 table the raster kernel reads: channel value (uint8)(c * 255.0f + 0.5f), alpha 255 (byte order r, g, b, a)
inline bool gradient_rgba8(const float *stops, int n, uint32_t *table /*[256]*/) {
    float r[256], g[256], b[256];
    if (!gradient(stops, n, 256, r, g, b)) return false;
    auto u8 = [](float c) -> uint32_t {
        volatile float p = c * 255.0f;                   // product and sum rounded one by one
        const float q = p + 0.5f;
        return q >= 0.5f ? (uint32_t)(uint8_t)q : 0u;    // (a NaN stop gives a NaN entry in the reference; here it is 0)
    };
    for (int i = 0; i < 256; ++i) table[i] = u8(r[i]) | (u8(g[i]) << 8) | (u8(b[i]) << 16) | 0xff000000u;
    return true;
}

// ---- the waterfall's viewport (src/panel/WaterfallPanel.cpp:161-219, csdr_hip.h "Waterfall viewport") ----------------------------------------
// The tap tables of a W x H view of the ring: which texels / scrolled rows a pixel column / row shows.  Exact integer arithmetic in int64; the
// only floats are the blend weights, (float)((double)numerator / (double)denominator).  Independent of waterfall_ofs.
struct ViewTap { int32_t first, count; float frac; int32_t half; };
constexpr int kViewLinear = 0, kViewPeak = 1, kViewMaxSide = 16384;
// pixel column px shows half 1 iff 2 px + 2 > W (the library's own definition: the reference's quads overlap by half a pixel, :185, :195, :206)
inline bool view_columns(int fft_size, int width, int mode, ViewTap *t) {
    if (!t || fft_size < 4 || width < 2 || width > kViewMaxSide || (mode != kViewLinear && mode != kViewPeak)) return false;
    const int64_t half = fft_size / 2, W = width, n0 = W / 2;
    for (int64_t px = 0; px < W; ++px) {
        const int h = 2 * px + 2 > W ? 1 : 0;
        ViewTap &o = t[px];
        o.half = h;
        if (mode == kViewLinear) {
            // u = 1/2 + (half - 2) num / (W + 1) (:186, :192-198, :205-211 with half_texel = 1 / half, sampled at the pixel centre)
            const int64_t num = h ? 2 * px + 2 - W : 2 * px + 1, den = 2 * (W + 1), n = (W + 1) + 2 * (half - 2) * num;
            o.first = (int32_t)(n / den);
            o.count = 2;
            o.frac = (float)((double)(n % den) / (double)den);
        } else {
            const int64_t nh = h ? W - n0 : n0, k = h ? px - n0 : px, a = k * half / nh, b = (k + 1) * half / nh;
            o.first = (int32_t)a;
            o.count = (int32_t)(b > a ? b - a : 1);
            o.frac = 0.0f;
        }
    }
    return true;
}
inline bool view_rows(int lines, int height, int mode, ViewTap *t) {
    if (!t || lines < 2 || lines > (1 << 20) || height < 1 || height > kViewMaxSide || (mode != kViewLinear && mode != kViewPeak)) return false;
    const int64_t L = lines, H = height;
    for (int64_t py = 0; py < H; ++py) {
        ViewTap &o = t[py];
        o.half = 0;
        if (mode == kViewLinear) {
            // t = (ofs + L (py + 1/2) / H) / L under GL_REPEAT, texel centres at (j + 1/2) / L: j = q + beta with n = L (2 py + 1) - H over 2 H
            const int64_t n = L * (2 * py + 1) - H, den = 2 * H;
            const int64_t q = n >= 0 ? n / den : -((-n + den - 1) / den);
            o.first = (int32_t)q;
            o.count = 2;
            o.frac = (float)((double)(n - q * den) / (double)den);
        } else {
            const int64_t a = py * L / H, b = (py + 1) * L / H;
            o.first = (int32_t)a;
            o.count = (int32_t)(b > a ? b - a : 1);
            o.frac = 0.0f;
        }
    }
    return true;
}

// ---- block / channel sizing rules of the reference's SDR thread (SoapySDRThread.cpp:668-693) ---------------
inline int optimal_channel_count(int64_t sample_rate) {
    if (sample_rate <= 500000) return 1;
    int64_t c = (int64_t)std::ceil((double)sample_rate / 500000.0);
    if (c % 2 == 1) c--;
    if (c < 2) c = 2;
    return (int)c;
}
inline int optimal_element_count(int64_t sample_rate, int fps, int num_channels) {
    int n = (int)std::floor((double)sample_rate / (double)fps);
    n = (int)(std::ceil((double)n / (double)num_channels) * num_channels);
    return n;
}

// ---- overlay planners: the reference's display arithmetic as records and csdr_overlay_prims (include/csdr_hip.h, "Overlay bank", a - e) -------
// NDC -> pixels, one rule for every planner, in double
inline int ndc_hb(double u, int W) { const double b = std::floor((u + 1.0) * 0.5 * (double)W); return b < 0.0 ? 0 : (b > (double)W ? W : (int)b); }
inline int ndc_vb(double v, int H) { const double b = std::floor((1.0 - v) * 0.5 * (double)H); return b < 0.0 ? 0 : (b > (double)H ? H : (int)b); }
inline uint8_t unit_byte(double c) { return (uint8_t)(int)(c * 255.0 + 0.5); }
inline bool view_ok(int w, int h) { return w >= 1 && w <= 16384 && h >= 1 && h <= 16384; }

// SpectrumPanel.cpp:171-277, with the reference's types: long long frequencies, long double steps, double m, float view sizes
inline int freq_scale(int64_t freq, int64_t bandwidth, int view_w, int view_h, double font_scale, csdr_freq_scale *out, csdr_freq_tick *ticks, int cap) {
    if (!out || (cap > 0 && !ticks) || cap < 0 || bandwidth < 1 || !view_ok(view_w, view_h) || !(font_scale > 0.0)) return CSDR_EINVAL;
    const float viewWidth = (float)view_w, viewHeight = (float)view_h;
    const long long leftFreq = (long long)((double)freq - ((double)bandwidth / 2.0));                 // :171
    const long long rightFreq = (long long)((double)leftFreq + (double)bandwidth);                    // :172
    if (rightFreq - leftFreq < 1) return CSDR_EINVAL;
    const long double span = (long double)(rightFreq - leftFreq);
    const long long hzStep = 1000000;
    long double mhzStep = (100000.0 / span) * 2.0;                                                   // :176
    double mhzVisualStep = 0.1;
    int precision = 1;
    auto narrow = [&]() { return mhzStep * 0.5 * viewWidth < 40 * font_scale; };
    if (narrow()) {                                                                                  // :184-216
        static const double ladder[7] = {0.25, 0.5, 1.0, 2.5, 5.0, 10.0, 50.0};
        for (int k = 0; k < 7 && (k == 0 || narrow()); ++k) { mhzStep = ((ladder[k] * 1000000.0) / span) * 2.0; mhzVisualStep = ladder[k]; }
    } else if (mhzStep * 0.5 * viewWidth > 350 * font_scale) {                                       // :217-221
        mhzStep = (10000.0 / span) * 2.0;
        mhzVisualStep = 0.01;
        precision = 2;
    }
    const long long firstMhz = (leftFreq / hzStep) * hzStep;                                         // :223, truncating
    const long double mhzStart = ((long double)(firstMhz - leftFreq) / span) * 2.0;
    long double currentMhz = truncl(floorl(firstMhz / (long double)1000000.0));
    out->step_mhz = mhzVisualStep; out->precision = precision; out->pad = 0;
    out->tick_top = 1.0 - (5.0 / viewHeight);                                                        // :229
    out->label_y = 1.0 - (16.0 / viewHeight) * font_scale; out->font_size = 12;                      // :228
    if (viewHeight > 135) { out->font_size = 16; out->label_y = 1.0 - (18.0 / viewHeight) * font_scale; }
    out->tick_rows = ndc_vb(out->tick_top, view_h); out->label_row = ndc_vb(out->label_y, view_h);
    int n = 0;
    long long turns = 0;
    for (double m = (double)(-1.0 + mhzStart), mMax = (double)(1.0 + ((mhzStart > 0) ? mhzStart : -mhzStart)); m <= mMax; m = (double)(m + mhzStep)) {    // :241
        if (++turns > (1 << 20)) return CSDR_EINVAL;
        if (m < -1.0) { currentMhz += mhzVisualStep; continue; }
        if (m > 1.0) break;
        if (n < cap) {
            csdr_freq_tick &t = ticks[n];
            double intpart;
            t.m = m; t.value = (double)currentMhz;
            t.major = std::modf((double)currentMhz, &intpart) < 0.001 ? 1 : 0;                       // :253-255
            t.column = ndc_hb(m, view_w);
            std::snprintf(t.label, sizeof t.label, "%.*Lf", precision, currentMhz);                  // :249
        }
        ++n;
        currentMhz += mhzVisualStep;
    }
    out->n_ticks = n;
    return n > cap ? CSDR_ERANGE : CSDR_OK;
}

// SpectrumPanel.cpp:117-147
inline int db_grid(float floor_value, float ceil_value, csdr_db_grid_range *ranges, int *n_ranges, double *p_out, int cap) {
    if (!ranges || !n_ranges || (cap > 0 && !p_out) || cap < 0 || !std::isfinite(floor_value) || !std::isfinite(ceil_value)) return CSDR_EINVAL;
    const double range = ceil_value - floor_value;                                                   // :119, a float difference
    static const double table[3][4] = {{90.0, 5000.0, 10.0, 100.0}, {20.0, 150.0, 10.0, 10.0}, {-20.0, 30.0, 10.0, 1.0}};
    int nr = 0, np = 0;
    for (const auto &i : table) {
        const double rangeMin = i[0], rangeMax = i[1], rangeTrans = i[2], rangeStep = i[3];
        if (!(range >= rangeMin && range <= rangeMax)) continue;
        double a = 1.0, p = 0;
        if (range <= rangeMin + rangeTrans) a *= (range - rangeMin) / rangeTrans;
        if (range >= rangeMax - rangeTrans) a *= (rangeTrans - (range - (rangeMax - rangeTrans))) / rangeTrans;
        csdr_db_grid_range &r = ranges[nr++];
        r.alpha = a; r.step = rangeStep; r.first = np; r.count = 0;
        for (double l = floor_value; l <= ceil_value + rangeStep; l += rangeStep) {                  // :141
            p += rangeStep / range;
            if (np < cap) p_out[np] = p;
            ++np; ++r.count;
        }
    }
    *n_ranges = nr;
    return np > cap ? CSDR_ERANGE : CSDR_OK;
}

// SpectrumPanel.cpp:281-303
inline int db_labels(float floor_value, float ceil_value, int fft_size, double db_offset, char *ceil_label, char *floor_label, int cap) {
    if (!ceil_label || !floor_label || cap < 1) return CSDR_EINVAL;
    ceil_label[0] = floor_label[0] = 0;
    if (ceil_value == floor_value || fft_size == 0) return CSDR_OK;
    const int a = std::snprintf(ceil_label, (size_t)cap, "%.1fdB", db_offset + 20.0 * std::log10(2.0 * (ceil_value) / (double)fft_size));
    const int b = std::snprintf(floor_label, (size_t)cap, "%.1fdB", db_offset + 20.0 * std::log10(2.0 * (floor_value) / (double)fft_size));
    return a >= cap || b >= cap ? CSDR_ERANGE : CSDR_OK;
}

// PrimaryGLContext.cpp:89-164, :168-197, in float as the reference
inline int demod_marker(int64_t demod_freq, int bandwidth, int sideband, int64_t center_freq, int64_t srate, int flags, int view_w, int view_h,
                        const uint8_t *rgb, csdr_demod_marker *out, csdr_overlay_prim *prims, int *n_prims) {
    if (!rgb || !out || !prims || !n_prims || srate < 1 || !view_ok(view_w, view_h) || sideband < CSDR_SIDEBAND_BOTH || sideband > CSDR_SIDEBAND_LSB) return CSDR_EINVAL;
    const float viewHeight = (float)view_h, viewWidth = (float)view_w;
    float uxPos = (float)(demod_freq - (center_freq - srate / 2)) / (float)srate;                    // :89
    uxPos = (float)((uxPos - 0.5) * 2.0);
    const float ofs = ((float)bandwidth) / (float)srate;                                             // :98
    const float ofsLeft = sideband != CSDR_SIDEBAND_USB ? ofs : 0, ofsRight = sideband != CSDR_SIDEBAND_LSB ? ofs : 0;
    const float labelHeight = (float)(20.0 / viewHeight);
    const float hPos = (float)(-1.0 + labelHeight);
    const int x0 = ndc_hb(uxPos - ofsLeft, view_w), x1 = ndc_hb(uxPos + ofsRight, view_w), ytop = ndc_vb(hPos + labelHeight, view_h);
    int n = 0;
    auto rect = [&](int x, int y, int w, int h, uint8_t r, uint8_t g, uint8_t b, double alpha, int mode) {
        prims[n++] = csdr_overlay_prim{x, y, w < 0 ? 0 : w, h < 0 ? 0 : h, {r, g, b, unit_byte(alpha)}, mode, -1, 0};
    };
    rect(x0, ytop, x1 - x0, view_h - ytop, 0, 0, 0, 0.35f, CSDR_OVL_OVER);                           // :110-134
    rect(x0, 0, x1 - x0, view_h, rgb[0], rgb[1], rgb[2], 0.2f, CSDR_OVL_ADD);                        // :136-145
    out->narrow = ofs * 2.0 < 16.0 / viewWidth ? 1 : 0;                                              // :147
    if (out->narrow) rect(x0, ytop, x1 - x0, view_h - ytop, rgb[0], rgb[1], rgb[2], 0.2f, CSDR_OVL_ADD);
    const int xc = ndc_hb(uxPos, view_w);
    if ((flags & CSDR_MARKER_CENTERLINE) && xc < view_w) rect(xc, 0, 1, view_h, rgb[0], rgb[1], rgb[2], 0.5, CSDR_OVL_ADD);      // :158-164
    *n_prims = n;
    out->ux = uxPos; out->ofs_left = ofsLeft; out->ofs_right = ofsRight; out->label_v = hPos;
    out->halign = sideband == CSDR_SIDEBAND_USB ? CSDR_ALIGN_LEFT : (sideband == CSDR_SIDEBAND_LSB ? CSDR_ALIGN_RIGHT : CSDR_ALIGN_CENTER);   // :191-197
    out->label_x = xc; out->label_y = ndc_vb(hPos, view_h);
    char letters[4];
    int nl = 0;
    if (flags & CSDR_MARKER_DELTA_LOCK) letters[nl++] = 'V';                                         // :170-182
    if (flags & CSDR_MARKER_RECORDING) letters[nl++] = 'R';
    if (flags & CSDR_MARKER_MUTED) letters[nl++] = 'M'; else if (flags & CSDR_MARKER_SOLO) letters[nl++] = 'S';
    letters[nl] = 0;
    std::snprintf(out->prefix, sizeof out->prefix, nl ? "[%s] " : "%s", letters);
    return CSDR_OK;
}

// one string as masked primitives (csdr_hip.h, "Overlay bank", e)
inline int text_prims(const csdr_glyph *glyphs, int n_glyphs, int line_height, const char *str, int x, int y, int halign, int valign, const uint8_t *rgba, int mode,
                      csdr_overlay_prim *out, int cap, int *n_out) {
    if (!str || !rgba || !n_out || n_glyphs < 0 || (n_glyphs > 0 && !glyphs) || (cap > 0 && !out) || cap < 0 || line_height < 0 || halign < CSDR_ALIGN_LEFT ||
        halign > CSDR_ALIGN_RIGHT || valign < CSDR_ALIGN_TOP || valign > CSDR_ALIGN_BOTTOM || mode < CSDR_OVL_OVER || mode > CSDR_OVL_COPY) return CSDR_EINVAL;
    auto find = [&](char c) -> const csdr_glyph * {
        for (int k = 0; k < n_glyphs; ++k) if (glyphs[k].id == (int)(unsigned char)c) return &glyphs[k];
        return nullptr;
    };
    auto floor_half = [](long long v) { return (v - (v < 0 ? 1 : 0)) / 2; };
    long long width = 0;
    for (const char *c = str; *c; ++c) if (const csdr_glyph *g = find(*c)) { if (g->w < 0 || g->h < 0) return CSDR_EINVAL; width += g->xadvance; }
    long long pen = halign == CSDR_ALIGN_LEFT ? x : (halign == CSDR_ALIGN_CENTER ? x - floor_half(width) : x - width);
    const long long top = valign == CSDR_ALIGN_TOP ? y : (valign == CSDR_ALIGN_CENTER ? y - floor_half(line_height) : (long long)y - line_height);
    int n = 0;
    for (const char *c = str; *c; ++c) {
        const csdr_glyph *g = find(*c);
        if (!g) continue;
        if (g->w > 0 && g->h > 0) {
            if (n < cap) out[n] = csdr_overlay_prim{(int32_t)(pen + g->xoffset), (int32_t)(top + g->yoffset), g->w, g->h, {rgba[0], rgba[1], rgba[2], rgba[3]}, mode, g->x, g->y};
            ++n;
        }
        pen += g->xadvance;
    }
    *n_out = n;
    return n > cap ? CSDR_ERANGE : CSDR_OK;
}

}  // namespace design
}  // namespace csdr
