// kernels_digital.hpp -- the digital lab (reference src/modules/modem/digital/, built there with ENABLE_DIGITAL_LAB): per-sample hard decisions of
// the modemcf constellations of ModemPSK / DPSK / ASK / QAM / BPSK / QPSK / OOK, and the fskdem symbols of ModemFSK, behind the front-end's
// resampled IQ.  One launch covers every digital slot and every block of a batch.
//
// Replaces (reference file:line): Modem{PSK,DPSK,ASK,QAM}.cpp ::demodulate (the modemcf_demodulate loop and updateDemodulatorLock),
// Modem{BPSK,QPSK,OOK}.cpp ::demodulate, ModemFSK.cpp:127-143 (inputBuffer, fskdem_demodulate per k samples).
//
// The constellations are computed here from their definitions (Gray-coded phase / amplitude levels, rectangular grids, unit mean energy); the
// decision rules are the demodulator's own, not nearest-point: the phase is offset and quantised by successive approximation, amplitude levels and
// the I / Q rails of a grid by successive-approximation thresholds each, DPSK quantises the phase difference to the previous input sample.
#pragma once
#include "common.hpp"
#include "kernels_demod.hpp"

namespace csdr {

enum DigScheme : int32_t { DIG_PSK = 0, DIG_DPSK, DIG_ASK, DIG_QAM, DIG_BPSK, DIG_QPSK, DIG_OOK, DIG_FSK, DIG_GMSK, DIG_TABLE };

constexpr int kDigThreads = 256;
constexpr int kDigFskMaxK = 2048;          // fskdem samples per symbol (its create rule: k <= 2^11)
constexpr int kDigStateFloats = 8;         // per constellation: r (2), x_hat (2), DPSK input phase, 3 spare

// one constellation's decision geometry (host-computed from the definition: csdr_digital.hip dig_geometry)
struct DigGeom {
    int32_t scheme;       // DigScheme
    int32_t m_i, m_q;     // bits on the phase / amplitude / I rail, bits on the Q rail (QAM)
    float alpha;          // PSK / DPSK: pi / M (half the phase step); ASK / QAM: the level step that gives unit mean energy
    float d_phi;          // PSK / DPSK: pi (1 - 1 / M), the phase offset taken off before quantising
    float step;           // PSK / DPSK: 2 pi / M
};

// one digital slot's work in one launch
struct DigJob {
    const float2 *iq;         // this batch's resampled IQ (n samples)
    int32_t n;                // samples of the batch
    int32_t nb;               // blocks of the batch
    const BlockPlan *plan;    // [nb + 1] block starts inside the batch (front-end plans; the standalone entry: one block)
    uint32_t *sym;            // symbols out: one per sample (constellations), one per whole symbol (FSK)
    float *bevm;              // [nb] per block: the EVM after the block (constellations)
    const float *st_rd;       // the active constellation's state before the batch (kDigStateFloats)
    float *st_wr;             // ... and after it (another copy: the first and the last workgroup may run at once)
    DigGeom g;
    // FSK
    int32_t k, K, M, carry, nsym, new_carry;     // samples per symbol, transform size, tones, carried samples in / out, whole symbols
    const uint32_t *map;      // [M] transform bin of each tone
    const float2 *stash_rd;   // [carry] samples carried in
    float2 *stash_wr;         // [new_carry] samples carried out
};

__host__ __device__ __forceinline__ uint32_t dig_gray_encode(uint32_t s) { return s ^ (s >> 1); }
__host__ __device__ __forceinline__ uint32_t dig_gray_decode(uint32_t s) {
    for (uint32_t k = s >> 1; k; k >>= 1) s ^= k;
    return s;
}

// successive approximation over m bits with reference steps 2^k alpha (k = m-1 .. 0): the offset-binary level index; *res is what is left of v
__host__ __device__ __forceinline__ uint32_t dig_linear(float v, int m, float alpha, float *res) {
    uint32_t s = 0;
    for (int k = m - 1; k >= 0; --k) {
        const float ref = (float)(1u << k) * alpha;
        s <<= 1;
        if (v > 0.0f) { s |= 1u; v -= ref; }
        else v += ref;
    }
    *res = v;
    return s;
}

// amplitude level of an offset-binary index on a rail of 2^m levels: (2 s - 2^m + 1) alpha
__host__ __device__ __forceinline__ float dig_level(uint32_t s, int m, float alpha) { return (float)(2 * (int)s - (1 << m) + 1) * alpha; }

__host__ __device__ __forceinline__ float2 dig_unit(uint32_t s, float step) {
    const float th = (float)s * step;
    return make_float2(cosf(th), sinf(th));
}

// one sample's hard decision.  phi_prev: DPSK's phase of the previous input sample; *phi gets this sample's.  *xhat: the re-modulated decision.
__host__ __device__ __forceinline__ uint32_t dig_decide(const DigGeom &g, float2 x, float phi_prev, float *phi, float2 *xhat) {
    constexpr double kPi = 3.14159265358979323846;
    float res;
    switch (g.scheme) {
    case DIG_PSK: {
        float th = atan2f(x.y, x.x) - g.d_phi;
        if (th < -kPi) th = (float)((double)th + 2.0 * kPi);
        const uint32_t s = dig_linear(th, g.m_i, g.alpha, &res);
        *xhat = dig_unit(s, g.step);
        return dig_gray_encode(s);
    }
    case DIG_DPSK: {
        const float th = atan2f(x.y, x.x);
        float d = (th - phi_prev) - g.d_phi;
        if (d > kPi) d = (float)((double)d - 2.0 * kPi);
        else if (d < -kPi) d = (float)((double)d + 2.0 * kPi);
        const uint32_t s = dig_linear(d, g.m_i, g.alpha, &res);
        *phi = th;
        const float t = th - res;
        *xhat = make_float2(cosf(t), sinf(t));
        return dig_gray_encode(s);
    }
    case DIG_ASK: {
        const uint32_t s = dig_linear(x.x, g.m_i, g.alpha, &res);
        *xhat = make_float2(dig_level(s, g.m_i, g.alpha), 0.0f);
        return dig_gray_encode(s);
    }
    case DIG_QAM: {
        const uint32_t si = dig_linear(x.x, g.m_i, g.alpha, &res), sq = dig_linear(x.y, g.m_q, g.alpha, &res);
        *xhat = make_float2(dig_level(si, g.m_i, g.alpha), dig_level(sq, g.m_q, g.alpha));
        return (dig_gray_encode(si) << g.m_q) | dig_gray_encode(sq);
    }
    case DIG_BPSK: {
        const uint32_t s = x.x > 0.0f ? 0u : 1u;
        *xhat = make_float2(s ? -1.0f : 1.0f, 0.0f);
        return s;
    }
    case DIG_QPSK: {
        const uint32_t s = (x.x > 0.0f ? 0u : 1u) | (x.y > 0.0f ? 0u : 2u);
        const float h = 0.70710678118654752f;
        *xhat = make_float2((s & 1u) ? -h : h, (s & 2u) ? -h : h);
        return s;
    }
    default: {   // DIG_OOK: a mark at sqrt(2), a space at 0
        const uint32_t s = x.x > 0.70710678118654752f ? 0u : 1u;
        *xhat = make_float2(s ? 0.0f : 1.41421356237309505f, 0.0f);
        return s;
    }
    }
}

__host__ __device__ __forceinline__ float dig_evm(float2 r, float2 xhat) {
    const float dx = xhat.x - r.x, dy = xhat.y - r.y;
    return sqrtf(dx * dx + dy * dy);
}

// FSK: the M tone bins of the K-point forward transform of one symbol's k samples (zero-padded to K), computed as M direct sums; the symbol is the
// first tone of largest magnitude.  One wave per symbol: lane l sums the samples l, l + 64, ... for every tone, then the wave reduces.
__device__ __forceinline__ uint32_t dig_fsk_symbol(const DigJob &j, int symbol, int lane) {
    const int64_t p0 = (int64_t)symbol * j.k;
    float best = 0.0f;
    uint32_t arg = 0;
    for (int t = 0; t < j.M; ++t) {
        const uint32_t bin = j.map[t];
        float re = 0.0f, im = 0.0f;
        for (int n = lane; n < j.k; n += 64) {
            const int64_t p = p0 + n;
            const float2 x = p < j.carry ? j.stash_rd[p] : j.iq[p - j.carry];
            const uint32_t e = (uint32_t)(((uint64_t)bin * (uint64_t)n) % (uint64_t)j.K);     // exp(-2 pi i bin n / K)
            const float a = -6.28318530717958648f * ((float)e / (float)j.K);
            const float s = sinf(a), c = cosf(a);
            re += x.x * c - x.y * s;
            im += x.x * s + x.y * c;
        }
        for (int o = 32; o > 0; o >>= 1) { re += __shfl_xor(re, o); im += __shfl_xor(im, o); }
        const float v = sqrtf(re * re + im * im);
        if (t == 0 || v > best) { best = v; arg = (uint32_t)t; }
    }
    return arg;
}

// grid (workgroups, jobs), kDigThreads threads.  Constellation job: workgroup x decides samples [x 256, + 256) -- one thread per sample, 8 B in,
// 4 B out -- and workgroup 0 also writes the per-block EVM (the block's last sample, decided again by the thread that reports it; an empty block
// repeats the state the object holds: the previous block's, or the one before the batch).  FSK job: wave w of workgroup x demodulates symbol
// 4 x + w; workgroup 0 also moves the samples that do not fill a symbol into the carry stash.
CSDR_KERNEL __launch_bounds__(kDigThreads) void digital_demod(const DigJob *__restrict__ jobs) {
    const DigJob &j = jobs[blockIdx.y];
    const int tid = threadIdx.x;
    if (j.g.scheme == DIG_FSK) {
        const int s = blockIdx.x * (kDigThreads / 64) + (tid >> 6), lane = tid & 63;
        if (s < j.nsym) {
            const uint32_t v = dig_fsk_symbol(j, s, lane);
            if (lane == 0) j.sym[s] = v;
        }
        if (blockIdx.x == 0) {
            const int64_t p0 = (int64_t)j.nsym * j.k;
            for (int i = tid; i < j.new_carry; i += kDigThreads) {
                const int64_t p = p0 + i;
                j.stash_wr[i] = p < j.carry ? j.stash_rd[p] : j.iq[p - j.carry];
            }
        }
        return;
    }
    const float2 r0 = make_float2(j.st_rd[0], j.st_rd[1]), xh0 = make_float2(j.st_rd[2], j.st_rd[3]);
    const float phi0 = j.st_rd[4];
    const int i = blockIdx.x * kDigThreads + tid;
    if (i < j.n) {
        const float2 x = j.iq[i];
        const float prev = (j.g.scheme == DIG_DPSK && i > 0) ? atan2f(j.iq[i - 1].y, j.iq[i - 1].x) : phi0;
        float phi = 0.0f;
        float2 xh;
        j.sym[i] = dig_decide(j.g, x, prev, &phi, &xh);
        if (i == j.n - 1) {
            j.st_wr[0] = x.x; j.st_wr[1] = x.y; j.st_wr[2] = xh.x; j.st_wr[3] = xh.y;
            j.st_wr[4] = j.g.scheme == DIG_DPSK ? phi : phi0;
        }
    }
    if (blockIdx.x == 0) {
        for (int bb = tid; bb < j.nb; bb += kDigThreads) {
            const int last = j.plan[bb + 1].j0 - 1;           // the last sample decided up to the end of this block
            float e;
            if (last < 0) e = dig_evm(r0, xh0);
            else {
                const float2 x = j.iq[last];
                const float prev = (j.g.scheme == DIG_DPSK && last > 0) ? atan2f(j.iq[last - 1].y, j.iq[last - 1].x) : phi0;
                float phi;
                float2 xh;
                (void)dig_decide(j.g, x, prev, &phi, &xh);
                e = dig_evm(x, xh);
            }
            j.bevm[bb] = e;
        }
    }
}

// ---- table-driven constellations (ModemAPSK / ModemSQAM / ModemST; liquid's arb and APSK demodulators): the points are caller data
// (csdr_constellation), the decision one of three rules -- the first nearest point, the same behind a fold into the first quadrant, or a ring slicer on |x| and a
// rounded phase index within the ring.  One launch covers every table slot and block of a batch.
constexpr int kTabThreads = 256;
constexpr int kTabMaxPoints = 256, kTabMaxRings = 8;

// one table as the kernel reads it (host-built from a csdr_constellation: csdr_digital.hip table_device); staged whole in LDS per workgroup
struct TableDev {
    int32_t rule, n_points, n_rings, pad;
    float2 points[kTabMaxPoints];          // by symbol
    float ring_slicer[kTabMaxRings];       // [n_rings - 1] used
    float ring_phase[kTabMaxRings];
    float ring_dphi[kTabMaxRings];         // (float)(2 pi / ring_size)
    int32_t ring_size[kTabMaxRings];
    int32_t ring_base[kTabMaxRings];       // points on the rings inside this one
    uint8_t inv[kTabMaxPoints];            // ring-ordered index -> symbol
};
static_assert(sizeof(TableDev) % 4 == 0 && offsetof(TableDev, points) % 16 == 0 && kTabMaxPoints % 8 == 0 && sizeof(TableDev) == 16 + 8 * kTabMaxPoints + 5 * 4 * kTabMaxRings + kTabMaxPoints, "TableDev is staged as dwords");

struct TableJob {
    const float2 *iq;         // this batch's resampled IQ (n samples)
    int32_t n, nb;            // samples, blocks of the batch
    const BlockPlan *plan;    // [nb + 1] block starts inside the batch
    uint32_t *sym;            // one symbol per sample
    float *bevm;              // [nb] the EVM after each block
    const float *st_rd;       // the deciding table's state before the batch (kDigStateFloats) ...
    float *st_wr;             // ... and after it (the other copy)
    const TableDev *tab;
};

// one sample's decision against the table in LDS; *xhat = points[symbol]
__device__ __forceinline__ uint32_t table_decide(const TableDev &t, float2 x, float2 *xhat) {
    uint32_t s = 0;
    if (t.rule != 1) {      // the first point at the least distance; every product and sum rounded on its own
        int np = t.n_points;
        uint32_t quad = 0;
        if (t.rule == 2) {  // folded into the first quadrant by the signs alone (exact), searched among the first quarter of the points
            const bool nr = x.x < 0.0f, ni = x.y < 0.0f;
            quad = (nr ? 2u : 0u) + (ni ? 1u : 0u);
            x = make_float2(nr ? -x.x : x.x, ni ? -x.y : x.y);
            np >>= 2;
        }
        // eight points a turn, their four LDS reads in flight together (one read a turn leaves the scan waiting on LDS latency); the array holds
        // kTabMaxPoints whatever np is, so a turn's reads stay inside it.  Strict "<" from +inf in index order: the first of the least
        float best = INFINITY;
        const float4 *pt = reinterpret_cast<const float4 *>(t.points);
        for (int i = 0; i < np; i += 8) {
            float4 q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = pt[(i >> 1) + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float px = (k & 1) ? q[k >> 1].z : q[k >> 1].x, py = (k & 1) ? q[k >> 1].w : q[k >> 1].y;
                const float dx = x.x - px, dy = x.y - py;
                const float d = rounded(dx * dx) + rounded(dy * dy);
                if (i + k < np && d < best) { best = d; s = (uint32_t)(i + k); }
            }
        }
        s += quad * (uint32_t)np;
    } else {
        constexpr double kTwoPi = 6.28318530717958647692;
        const float rad = sqrtf(rounded(x.x * x.x) + rounded(x.y * x.y));
        int l = t.n_rings - 1;
        for (int i = t.n_rings - 2; i >= 0; --i) if (rad < t.ring_slicer[i]) l = i;      // the first ring whose slicer lies above
        float th = atan2f(x.y, x.x);
        if (th < 0.0f) th = (float)((double)th + kTwoPi);
        const int p = t.ring_size[l];
        int j = (int)roundf((th - t.ring_phase[l]) / t.ring_dphi[l]) % p;
        if (j < 0) j += p;
        s = t.inv[t.ring_base[l] + j];
    }
    *xhat = t.points[s];
    return s;
}

// grid (workgroups, jobs), kTabThreads threads, sizeof(TableDev) bytes of dynamic LDS.  Workgroup x of a job stages the job's table in LDS (every
// lane of a wave then reads the same address: a broadcast, no bank conflicts) and decides samples [x 256, + 256), one thread per sample; workgroup 0
// also writes the per-block EVM, deciding each block's last sample again (an empty block repeats the state the object holds), as digital_demod.
CSDR_KERNEL __launch_bounds__(kTabThreads) void table_demod(const TableJob *__restrict__ jobs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TableJob &j = jobs[blockIdx.y];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * kTabThreads;
    if (blockIdx.x != 0 && i0 >= j.n) return;              // (the whole workgroup: the grid is as wide as the batch's longest job)
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(j.tab);
        uint32_t *dst = reinterpret_cast<uint32_t *>(smem);
        for (int w = tid; w < (int)(sizeof(TableDev) / 4); w += kTabThreads) dst[w] = src[w];
    }
    __syncthreads();
    const TableDev &t = *reinterpret_cast<const TableDev *>(smem);
    const int i = i0 + tid;
    if (i < j.n) {
        const float2 x = j.iq[i];
        float2 xh;
        j.sym[i] = table_decide(t, x, &xh);
        if (i == j.n - 1) { j.st_wr[0] = x.x; j.st_wr[1] = x.y; j.st_wr[2] = xh.x; j.st_wr[3] = xh.y; }
    }
    if (blockIdx.x == 0) {
        const float2 r0 = make_float2(j.st_rd[0], j.st_rd[1]), xh0 = make_float2(j.st_rd[2], j.st_rd[3]);
        for (int bb = tid; bb < j.nb; bb += kTabThreads) {
            const int last = j.plan[bb + 1].j0 - 1;
            float e;
            if (last < 0) e = dig_evm(r0, xh0);
            else {
                const float2 x = j.iq[last];
                float2 xh;
                (void)table_decide(t, x, &xh);
                e = dig_evm(x, xh);
            }
            j.bevm[bb] = e;
        }
    }
}

// ---- GMSK (ModemGMSK.cpp:116-134, gmskdem(k, m, BT)): per symbol of k samples, the phase differences arg(conj(x_prev) x) go through the
// receive filter (h_len = 2 k m + 1 taps, no equaliser) and the filter output after the symbol's FIRST push is decided by its sign (> 0: 1).
// Two launches cover every GMSK slot and block of a batch.  gmsk_phase writes each slot's phase-difference stream: the h_len - 1
// values carried from the previous batch, then every block's processed range in order.  A block's range is the I k samples its I symbols read
// from the block's start; samples at or past the block's end read as zero, and the first sample's x_prev is the last sample the previous symbol
// read.  gmsk_decide then takes one wave per symbol over that stream and keeps the last h_len - 1 values for the next batch.
constexpr int kGmskThreads = 256;

struct GmskBlock {
    int32_t off;     // stream position of the block's first processed sample ([nb]: the stream's length)
    int32_t j0, n;   // the block's samples in the batch IQ
    int32_t prev;    // x_prev of its first processed sample: a batch IQ index, -1 (zero: a sample past an earlier block's end) or -2 (the carried
                     // x_prime); [nb]: the x_prime after the batch
};

struct GmskJob {
    const float2 *iq;          // this batch's resampled IQ
    const GmskBlock *blk;      // [nb + 1]
    int32_t nb, L, k, nsym;    // blocks, taps, samples per symbol, symbols of the batch
    const float *h;            // [L] receive filter
    const float *hist_rd;      // [L - 1] phase differences carried in (oldest first), then x_prime (2)
    float *hist_wr;            // the same after the batch (the other copy)
    float *phi;                // [blk[nb].off] the phase-difference stream
    uint32_t *sym;             // [nsym] decisions
    float *soft;               // [nsym] filter outputs, or null
};

// arg(conj(a) b) as the reference's object evaluates it: re = a.x b.x + a.y b.y, im = a.x b.y - a.y b.x -- with an exact zero operand the signs
// of the zero products decide between 0 and pi
__host__ __device__ __forceinline__ float gmsk_phase_diff(float2 a, float2 b) {
    const float re = a.x * b.x + a.y * b.y, im = a.x * b.y - a.y * b.x;
    return atan2f(im, re);
}

__device__ __forceinline__ float2 gmsk_sample(const GmskJob &j, const GmskBlock &bk, int u) {
    return u < bk.n ? j.iq[bk.j0 + u] : make_float2(0.0f, 0.0f);
}

__device__ __forceinline__ float2 gmsk_prev_of(const GmskJob &j, int32_t prev) {
    if (prev >= 0) return j.iq[prev];
    if (prev == -2) return make_float2(j.hist_rd[j.L - 1], j.hist_rd[j.L]);
    return make_float2(0.0f, 0.0f);
}

// grid (workgroups, jobs), kGmskThreads threads: one thread per stream position
CSDR_KERNEL __launch_bounds__(kGmskThreads) void gmsk_phase(const GmskJob *__restrict__ jobs) {
    const GmskJob &j = jobs[blockIdx.y];
    const int t = blockIdx.x * kGmskThreads + threadIdx.x;
    if (t == 0) {
        const float2 xp = gmsk_prev_of(j, j.blk[j.nb].prev);
        j.hist_wr[j.L - 1] = xp.x; j.hist_wr[j.L] = xp.y;
    }
    const int n_stream = j.blk[j.nb].off;
    if (t >= n_stream) return;
    if (t < j.L - 1) { j.phi[t] = j.hist_rd[t]; return; }
    int lo = 0, hi = j.nb - 1;                       // the last block starting at or before t (empty blocks share the next one's start)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (j.blk[mid].off <= t) lo = mid;
        else hi = mid - 1;
    }
    const GmskBlock bk = j.blk[lo];
    const int u = t - bk.off;
    const float2 x = gmsk_sample(j, bk, u), xp = u == 0 ? gmsk_prev_of(j, bk.prev) : gmsk_sample(j, bk, u - 1);
    j.phi[t] = gmsk_phase_diff(xp, x);
}

// grid (workgroups, jobs), kGmskThreads threads: wave w of workgroup x decides symbol 4 x + w, lanes striding the taps; workgroup 0 also keeps
// the stream's last L - 1 values
CSDR_KERNEL __launch_bounds__(kGmskThreads) void gmsk_decide(const GmskJob *__restrict__ jobs) {
    const GmskJob &j = jobs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int s = blockIdx.x * (kGmskThreads / 64) + (tid >> 6);
    if (s < j.nsym) {
        const float *x = j.phi + (j.L - 1) + (int64_t)s * j.k;       // the symbol's first push: h[i] meets the value i pushes before it
        float acc = 0.0f;
        for (int i = lane; i < j.L; i += 64) acc += j.h[i] * x[-i];
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) {
            j.sym[s] = acc > 0.0f ? 1u : 0u;
            if (j.soft) j.soft[s] = acc;
        }
    }
    if (blockIdx.x == 0) {
        const float *src = j.phi + (j.blk[j.nb].off - (j.L - 1));
        for (int i = tid; i < j.L - 1; i += kGmskThreads) j.hist_wr[i] = src[i];
    }
}

}  // namespace csdr
