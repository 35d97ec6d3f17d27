// csdr_digital.hip -- the digital lab (reference src/modules/modem/digital/): configuration of digital slots, their per-batch plan and launch behind
// the bank's front-end, the result fetches, csdr_digital_run (the decision kernel alone), csdr_gmsk_run (the GMSK kernels alone), the table-driven slots
// (csdr_bank_configure_table_slot, csdr_design_rings, csdr_table_run).  Kernels:
// kernels_digital.hpp; DESIGN 15.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "csdr_objects.hpp"
#include "design.hpp"
#include "kernels_digital.hpp"

using namespace csdr;

namespace csdr {

constexpr int kDigRecords = 8;               // constellation objects per modem: ModemPSK.cpp:6-13 and alike create eight (QAM seven)

struct DigSlot {
    csdr_digital_params p{};                 // defaults applied
    int idx = 0;                             // the constellation record in use (log2 cons - 1; QAM log2 cons - 2)
    DigGeom g{};
    float sens = -1.0f;                      // lock sensitivity (updateDemodulatorLock's second argument); < 0: FSK, no lock
    int k = 0, K = 0, M = 0;                 // FSK: samples per symbol, transform size, tones
    int carry = 0, stash_cur = 0;            // FSK: samples held (kit->inputBuffer), which stash copy holds them
    int st_cur[kDigRecords] = {0};           // which copy of each constellation's state is current
    void *mem = nullptr;                     // device: sym [cap_sym] | bevm [max_blocks] | st [8][2][8] | stash [2][kDigFskMaxK] | map [M]; GMSK: sym [cap_sym] |
                                             // taps | history | plan | phase differences, nothing of the others; table slot: sym | bevm | st | tables
    uint32_t *sym = nullptr;
    float *bevm = nullptr, *st = nullptr;
    float2 *stash = nullptr;
    uint32_t *map = nullptr;
    int cap_sym = 0;
    // the last execute
    std::vector<csdr_digital_result> res;
    int nsym = 0;
    bool ran = false;                        // the kernel ran for it (else every block repeats the state before the batch)
    int run_idx = 0, run_cons = 0;
    // planned by bank_digital_plan, launched by bank_digital_launch
    int n = 0, new_carry = 0, nsym_plan = 0;
    // GMSK: gmskdem(gk = sps, gm = fdelay, BT = bw), gL = 2 gk gm + 1 taps
    int gk = 0, gm = 0, gL = 0, hist_cur = 0;
    int64_t gcarry = 0;                      // kit->inputBuffer.size() (only its count is ever used) before the batch ...
    int64_t gcarry_new = 0;                  // ... and after it: planned, committed when the batch launches (a rejected batch changes nothing)
    float *gh = nullptr, *ghist = nullptr;   // device (inside mem): taps [gL] | history [2][gL + 1] (gL - 1 phase differences, x_prime)
    GmskBlock *gblk_d = nullptr;             // device: the batch's plan [max_blocks + 1]
    float *gphi = nullptr;                   // device: the batch's phase-difference stream [cap_phi]
    int64_t cap_phi = 0;
    std::vector<GmskBlock> gblk;             // the batch's plan [NB + 1]
    // table slot (CSDR_DIGITAL_TABLE): the reference's per-"cons" objects; idx picks one, its state is record idx of st
    std::vector<int> tab_cons;               // n_points of each table
    std::vector<float> tab_sens;
    TableDev *tab_d = nullptr;               // device (inside mem): [tab_cons.size()]
    ~DigSlot() { if (mem) (void)hipFree(mem); }
};

}  // namespace csdr

static bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }
static int ilog2(int v) { int m = 0; while ((1 << m) < v) ++m; return m; }

// defaults of the reference constructors (ModemPSK.cpp:6-15 cons = 2, ModemQAM cons = 4, ModemFSK.cpp:7-12 bps 1, sps 9600, bw 0.45)
static int dig_normalise(const csdr_digital_params *in, csdr_digital_params *out) {
    *out = *in;
    if (in->kind < CSDR_DIGITAL_PSK || in->kind > CSDR_DIGITAL_GMSK) return fail(CSDR_EINVAL, "digital kind %d", in->kind);
    if (in->kind == CSDR_DIGITAL_GMSK) {      // ModemGMSK.cpp:7-10: sps 4, fdelay 3, ebf 0.3
        if (!out->sps) out->sps = 4;
        if (!out->fdelay) out->fdelay = 3;
        if (out->bw == 0.0f) out->bw = 0.3f;
        out->cons = 0; out->bps = 0;
        // gmskdem_create returns no object for k < 2, m < 1 or BT outside (0, 1); beyond the settings' ranges (sps 2..512, fdelay 1..128) the
        // filter length is walled off
        if (out->sps < 2 || out->fdelay < 1 || !(out->bw > 0.0f && out->bw < 1.0f))
            return fail(CSDR_EUNSUPPORTED, "GMSK sps %d / fdelay %d / ebf %g: gmskdem_create builds no demodulator", out->sps, out->fdelay, (double)out->bw);
        if (out->sps > 512 || out->fdelay > 128) return fail(CSDR_EUNSUPPORTED, "GMSK sps %d / fdelay %d beyond the settings' ranges (512, 128)", out->sps, out->fdelay);
        return CSDR_OK;
    }
    if (in->kind == CSDR_DIGITAL_FSK) {
        if (!out->bps) out->bps = 1;
        if (!out->sps) out->sps = 9600;
        if (out->bw == 0.0f) out->bw = 0.45f;
        out->cons = 0;
        // (bps above 16, the reference's largest option: 2^bps tones in at most 4 x 2048 transform bins, whose map cannot be unique)
        if (out->bps < 1 || out->bps > 16 || out->sps < 1) return fail(CSDR_EUNSUPPORTED, "FSK bps %d / sps %d: no demodulator for it", out->bps, out->sps);
        return CSDR_OK;
    }
    out->bps = 0; out->sps = 0; out->bw = 0.0f;
    if (in->kind == CSDR_DIGITAL_BPSK || in->kind == CSDR_DIGITAL_OOK) out->cons = 2;
    else if (in->kind == CSDR_DIGITAL_QPSK) out->cons = 4;
    else if (!out->cons) out->cons = in->kind == CSDR_DIGITAL_QAM ? 4 : 2;
    return CSDR_OK;
}

// the decision geometry of a constellation, from its definition:
//   PSK / DPSK (M = 2^m): points exp(2 pi i s / M), Gray-numbered; quantising steps 2^k pi / M; the phase offset pi (1 - 1/M)
//   ASK: levels (2 s - M + 1) alpha with unit mean energy: alpha^2 (M^2 - 1) / 3 = 1
//   QAM: a 2^m_i x 2^m_q grid (m_i = ceil(m / 2)) of such levels on each rail, unit mean energy: alpha^2 (M_i^2 + M_q^2 - 2) / 3 = 1
static int dig_geometry(const csdr_digital_params &p, DigGeom *g, int *idx, float *sens) {
    memset(g, 0, sizeof *g);
    const int kind = p.kind, cons = p.cons;
    switch (kind) {
    case CSDR_DIGITAL_PSK: case CSDR_DIGITAL_DPSK: case CSDR_DIGITAL_ASK:
        if (!pow2_in(cons, 2, 256)) return fail(CSDR_EUNSUPPORTED, "cons %d: the reference offers 2 .. 256", cons);
        break;
    case CSDR_DIGITAL_QAM:
        if (!pow2_in(cons, 4, 256)) return fail(CSDR_EUNSUPPORTED, "QAM cons %d: the reference offers 4 .. 256", cons);
        break;
    default: break;
    }
    const int m = ilog2(cons), M = 1 << m;
    *idx = 0;
    *sens = 0.005f;
    switch (kind) {
    case CSDR_DIGITAL_PSK: case CSDR_DIGITAL_DPSK:
        g->scheme = kind == CSDR_DIGITAL_PSK ? DIG_PSK : DIG_DPSK;
        g->m_i = m;
        g->alpha = (float)(M_PI / M);
        g->d_phi = (float)(M_PI * (1.0 - 1.0 / M));
        g->step = (float)(2.0 * M_PI / M);
        *idx = m - 1;
        break;
    case CSDR_DIGITAL_ASK:
        g->scheme = DIG_ASK;
        g->m_i = m;
        g->alpha = (float)std::sqrt(3.0 / ((double)M * M - 1.0));
        *idx = m - 1;
        break;
    case CSDR_DIGITAL_QAM: {
        g->scheme = DIG_QAM;
        g->m_i = (m + 1) / 2; g->m_q = m / 2;
        const double mi = (double)(1 << g->m_i), mq = (double)(1 << g->m_q);
        g->alpha = (float)std::sqrt(3.0 / (mi * mi + mq * mq - 2.0));
        *idx = m - 2;
        *sens = 0.5f;
        break;
    }
    case CSDR_DIGITAL_BPSK: g->scheme = DIG_BPSK; break;
    case CSDR_DIGITAL_QPSK: g->scheme = DIG_QPSK; *sens = 0.8f; break;
    case CSDR_DIGITAL_OOK: g->scheme = DIG_OOK; break;
    case CSDR_DIGITAL_GMSK: g->scheme = DIG_GMSK; *sens = -1.0f; break;
    default: g->scheme = DIG_FSK; *sens = -1.0f; break;
    }
    return CSDR_OK;
}

// fskdem's demodulator geometry for M = 2^bps tones spread over `bw` (fraction of the rate), k samples per symbol: the transform size K in
// [k, max(16, 4k)] whose bin spacing comes nearest a whole number of bins per tone step (the first such K), and each tone's bin, rounded.
// Refused where fskdem_create returns no object -- k outside [2, 2048] (its message says [2^bps, 2048], its test is [2, 2048]: fewer samples than
// tones is built and run), bw outside (0, 0.5) -- and where the tones' bin map is not unique (the reference prints an error and goes on).
static int dig_fsk_plan(int bps, int k, float bw, int *K_out, std::vector<uint32_t> *map) {
    if (k < 2 || k > kDigFskMaxK) return fail(CSDR_EUNSUPPORTED, "FSK: %d samples per symbol outside [2, %d]", k, kDigFskMaxK);
    if (!(bw > 0.0f && bw < 0.5f)) return fail(CSDR_EUNSUPPORTED, "FSK: bandwidth %g outside (0, 0.5)", (double)bw);
    const int M = 1 << bps;
    const float M2 = 0.5f * (float)(M - 1);
    const float df = bw / M2;
    float err_min = 1e9f;
    int K = k;
    const int K_max = std::max(16, 4 * k);
    for (int Kh = k; Kh <= K_max; ++Kh) {
        const float v = 0.5f * df * (float)Kh;
        const float err = std::fabs(std::round(v) - v);
        if (Kh == k || err < err_min) { K = Kh; err_min = err; }
        if (err < 1e-6f) break;
    }
    map->resize(M);
    for (int s = 0; s < M; ++s) {
        const float freq = ((float)s - M2) * bw / M2;
        const float idx = freq * (float)K;
        (*map)[s] = (uint32_t)(idx < 0.0f ? std::round(idx + (float)K) : std::round(idx));
        if (s && (*map)[s] == (*map)[s - 1]) return fail(CSDR_EUNSUPPORTED, "FSK: tones %d and %d share transform bin %u (bw %g too small)", s - 1, s, (*map)[s], (double)bw);
    }
    *K_out = K;
    return CSDR_OK;
}

// checkSampleRate: ModemDigital.cpp:21-26 (at least MIN_BANDWIDTH), ModemFSK.cpp:19-28 (at least 2^bps samples per symbol, else 2 bps sps)
static int64_t dig_check_rate(const csdr_digital_params &p, int64_t rate) {
    if (p.kind == CSDR_DIGITAL_FSK) return ((double)rate / (double)p.sps < std::pow(2.0, p.bps)) ? (int64_t)2 * p.bps * p.sps : rate;
    return rate < 500 ? 500 : rate;
}

// everything a modem of these settings needs, or the refusal
static int dig_setup(const csdr_digital_params *in, int64_t rate, DigSlot *d, std::vector<uint32_t> *map) {
    if (int rc = dig_normalise(in, &d->p)) return rc;
    if (int rc = dig_geometry(d->p, &d->g, &d->idx, &d->sens)) return rc;
    if (d->p.kind == CSDR_DIGITAL_FSK) {
        const int64_t k = rate / d->p.sps;                                   // ModemFSK.cpp:99 (unsigned int)(sampleRate / sps)
        if (k > kDigFskMaxK || k < 2) return fail(CSDR_EUNSUPPORTED, "FSK: %lld samples per symbol outside [2, %d]", (long long)k, kDigFskMaxK);
        if (int rc = dig_fsk_plan(d->p.bps, (int)k, d->p.bw, &d->K, map)) return rc;
        d->k = (int)k; d->M = 1 << d->p.bps;
    }
    if (d->p.kind == CSDR_DIGITAL_GMSK) { d->gk = d->p.sps; d->gm = d->p.fdelay; d->gL = 2 * d->gk * d->gm + 1; }
    return CSDR_OK;
}

static int dig_cons_of(const DigSlot &d) { return d.p.kind == CSDR_DIGITAL_FSK ? d.M : d.p.kind == CSDR_DIGITAL_GMSK ? 2 : d.p.cons; }

extern "C" int csdr_bank_configure_digital_slot(csdr_bank *b, int slot, const csdr_demod_params *p, const csdr_digital_params *dp, const csdr_post *post) {
    DeviceScope dev__(b ? b->ctx : nullptr);
    if (!b || !p || !dp || !post) return fail(CSDR_EINVAL, "null argument");
    if (p->modem != CSDR_MODEM_DIGITAL) return fail(CSDR_EINVAL, "csdr_bank_configure_digital_slot: modem must be CSDR_MODEM_DIGITAL");
    if (slot < 0 || slot >= b->max_demods) return fail(CSDR_EINVAL, "slot out of range");
    if (p->bandwidth <= 0) return fail(CSDR_EINVAL, "bad rates");
    auto d = std::make_shared<DigSlot>();
    csdr_digital_params np;
    if (int rc = dig_normalise(dp, &np)) return rc;
    const int64_t rate = dig_check_rate(np, p->bandwidth);
    if (rate > INT32_MAX) return fail(CSDR_EINVAL, "modem rate %lld", (long long)rate);
    std::vector<uint32_t> map;
    if (int rc = dig_setup(dp, rate, d.get(), &map)) return rc;
    csdr_demod_params q = *p;
    q.bandwidth = (int32_t)rate;
    if (int rc = bank_configure_slot(b, slot, &q, post)) return rc;      // (resets the slot, its digital stage included)
    SlotHost &s = b->slots[slot];
    const bool gmsk = d->gL > 0;
    d->cap_sym = s.cfg.cap_iq;
    if (gmsk) {
        // ModemGMSK's count c stays at or below n_max (k - 1) + k for blocks of at most n_max samples (c' = S - k ceil(floor(S / k) / k) <=
        // S (k - 1) / k + 1 with S = c + n), and a batch reads c_before + (its samples) - c_after of them: the stream and the decisions of any
        // batch fit these sizes, fixed here once
        const int64_t k = d->gk, n_max = (s.cfg.cap_iq - 64 - b->max_blocks) / std::max(1, b->max_blocks) + 2;
        const int64_t reads = n_max * (k - 1) + k + s.cfg.cap_iq;
        d->cap_phi = d->gL - 1 + reads;
        d->cap_sym = (int)(reads / k + 1);
    }
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_sym = carve((size_t)d->cap_sym * sizeof(uint32_t)), o_bevm = carve(gmsk ? 0 : (size_t)b->max_blocks * sizeof(float));
    const size_t o_st = carve(gmsk ? 0 : (size_t)kDigRecords * 2 * kDigStateFloats * sizeof(float)), o_stash = carve(gmsk ? 0 : (size_t)2 * kDigFskMaxK * sizeof(float2));
    const size_t o_map = carve(gmsk ? 0 : std::max<size_t>(1, map.size()) * sizeof(uint32_t));
    const size_t o_gh = carve((size_t)d->gL * sizeof(float)), o_ghist = carve((size_t)2 * (d->gL + 1) * sizeof(float));
    const size_t o_gblk = carve(gmsk ? ((size_t)b->max_blocks + 1) * sizeof(GmskBlock) : 0), o_gphi = carve((size_t)d->cap_phi * sizeof(float));
    std::vector<float> taps;
    if (d->gL) taps = design::gmsk_rx_taps((unsigned)d->gk, (unsigned)d->gm, d->p.bw);
    if (hipMalloc(&d->mem, off) != hipSuccess) { d->mem = nullptr; s.configured = false; return fail(CSDR_ENOMEM, "digital slot of %zu bytes", off); }
    char *base = (char *)d->mem;
    d->sym = (uint32_t *)(base + o_sym); d->bevm = (float *)(base + o_bevm); d->st = (float *)(base + o_st);
    d->stash = (float2 *)(base + o_stash); d->map = (uint32_t *)(base + o_map);
    d->gh = (float *)(base + o_gh); d->ghist = (float *)(base + o_ghist);
    d->gblk_d = (GmskBlock *)(base + o_gblk); d->gphi = (float *)(base + o_gphi);
    // modemcf_create: r = x_hat = 0 (EVM 0), DPSK phase 0; fskdem: an empty input buffer.  A failure leaves the slot unconfigured, as above.
    // gmskdem_create: x_prime = 0 and an empty filter window (zeros)
    if (hipMemset(d->mem, 0, off) != hipSuccess || (!map.empty() && hipMemcpy(d->map, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) ||
        (!taps.empty() && hipMemcpy(d->gh, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
        s.configured = false;
        return fail(CSDR_EHIP, "digital slot initialisation: %s", hipGetErrorString(hipGetLastError()));
    }
    s.dig = d;
    return CSDR_OK;
}

// a caller's constellation as the kernel reads it, or the refusal
static int table_device(const csdr_constellation &c, TableDev *t, float *sens) {
    memset(t, 0, sizeof *t);
    if (c.rule != CSDR_TABLE_NEAREST && c.rule != CSDR_TABLE_RINGS && c.rule != CSDR_TABLE_QUADRANT) return fail(CSDR_EINVAL, "constellation rule %d", c.rule);
    if (!pow2_in(c.n_points, 2, CSDR_TABLE_MAX_POINTS)) return fail(CSDR_EINVAL, "constellation of %d points: a power of two in 2 .. 256", c.n_points);
    if (!(c.sensitivity >= 0.0f) || !std::isfinite(c.sensitivity)) return fail(CSDR_EINVAL, "constellation sensitivity %g", (double)c.sensitivity);
    *sens = c.sensitivity == 0.0f ? 0.005f : c.sensitivity;
    t->rule = c.rule; t->n_points = c.n_points;
    for (int i = 0; i < c.n_points; ++i) {
        if (!std::isfinite(c.points[2 * i]) || !std::isfinite(c.points[2 * i + 1])) return fail(CSDR_EINVAL, "constellation point %d is not finite", i);
        t->points[i] = make_float2(c.points[2 * i], c.points[2 * i + 1]);
    }
    if (c.rule == CSDR_TABLE_NEAREST) return CSDR_OK;
    if (c.rule == CSDR_TABLE_QUADRANT) {       // the fold's premise: quadrant q of the table is the first quadrant's points under q's sign changes
        const int m = c.n_points / 4;
        if (m < 1) return fail(CSDR_EINVAL, "a folded constellation needs at least 4 points");
        for (int i = 0; i < m; ++i) {
            const float2 a = t->points[i];
            const float2 w[3] = {make_float2(a.x, -a.y), make_float2(-a.x, a.y), make_float2(-a.x, -a.y)};
            for (int q = 1; q < 4; ++q) {
                const float2 p = t->points[i + q * m];
                if (p.x != w[q - 1].x || p.y != w[q - 1].y) return fail(CSDR_EINVAL, "point %d is not point %d folded into quadrant %d", i + q * m, i, q);
            }
        }
        return CSDR_OK;
    }
    if (c.n_rings < 1 || c.n_rings > CSDR_TABLE_MAX_RINGS) return fail(CSDR_EINVAL, "constellation of %d rings: 1 .. 8", c.n_rings);
    t->n_rings = c.n_rings;
    int base = 0;
    for (int l = 0; l < c.n_rings; ++l) {
        const int p = c.ring_size[l];
        if (p < 1 || p > c.n_points - base) return fail(CSDR_EINVAL, "ring %d of %d points: the rings must hold the %d points between them", l, p, c.n_points);
        if (!std::isfinite(c.ring_phase[l])) return fail(CSDR_EINVAL, "ring %d: phase is not finite", l);
        if (l + 1 < c.n_rings && !(c.ring_slicer[l] > (l ? c.ring_slicer[l - 1] : 0.0f) && std::isfinite(c.ring_slicer[l])))
            return fail(CSDR_EINVAL, "ring slicer %d = %g does not ascend", l, (double)c.ring_slicer[l]);
        t->ring_size[l] = p; t->ring_base[l] = base;
        t->ring_phase[l] = c.ring_phase[l];
        t->ring_slicer[l] = l + 1 < c.n_rings ? c.ring_slicer[l] : 0.0f;
        t->ring_dphi[l] = (float)(2.0 * M_PI / (double)p);
        base += p;
    }
    if (base != c.n_points) return fail(CSDR_EINVAL, "the rings hold %d points of %d", base, c.n_points);
    bool seen[CSDR_TABLE_MAX_POINTS] = {false};
    for (int s = 0; s < c.n_points; ++s) {
        const int k = c.ring_map[s];
        if (k >= c.n_points || seen[k]) return fail(CSDR_EINVAL, "ring_map is not a permutation (symbol %d -> %d)", s, k);
        seen[k] = true;
        t->inv[k] = (uint8_t)s;
    }
    return CSDR_OK;
}

extern "C" int csdr_design_rings(const float *points, int n_points, csdr_constellation *out) {
    if (!points || !out) return fail(CSDR_EINVAL, "null argument");
    design::RingPlan r;
    if (!design::design_rings(points, n_points, &r))
        return fail(CSDR_EINVAL, "csdr_design_rings: %d points are not 2^k (2 .. 256) distinct points on at most 8 concentric, evenly spaced rings", n_points);
    memset(out, 0, sizeof *out);
    out->rule = CSDR_TABLE_RINGS; out->n_points = n_points; out->n_rings = r.n_rings;
    memcpy(out->points, points, (size_t)2 * n_points * sizeof(float));
    for (int l = 0; l < r.n_rings; ++l) {
        out->ring_size[l] = r.size[l]; out->ring_radius[l] = r.radius[l]; out->ring_phase[l] = r.phase[l]; out->ring_slicer[l] = r.slicer[l];
    }
    memcpy(out->ring_map, r.map, (size_t)n_points);
    return CSDR_OK;
}

extern "C" int csdr_bank_configure_table_slot(csdr_bank *b, int slot, const csdr_demod_params *p, const csdr_constellation *tables, int n_tables,
                                              const csdr_post *post) {
    DeviceScope dev__(b ? b->ctx : nullptr);
    if (!b || !p || !tables || !post) return fail(CSDR_EINVAL, "null argument");
    if (p->modem != CSDR_MODEM_DIGITAL) return fail(CSDR_EINVAL, "csdr_bank_configure_table_slot: modem must be CSDR_MODEM_DIGITAL");
    if (slot < 0 || slot >= b->max_demods) return fail(CSDR_EINVAL, "slot out of range");
    if (p->bandwidth <= 0) return fail(CSDR_EINVAL, "bad rates");
    static_assert(CSDR_TABLE_MAX_TABLES <= kDigRecords, "one state record per table");
    if (n_tables < 1 || n_tables > CSDR_TABLE_MAX_TABLES) return fail(CSDR_EINVAL, "%d tables: 1 .. %d", n_tables, CSDR_TABLE_MAX_TABLES);
    auto d = std::make_shared<DigSlot>();
    std::vector<TableDev> th((size_t)n_tables);
    d->tab_cons.resize((size_t)n_tables); d->tab_sens.resize((size_t)n_tables);
    for (int i = 0; i < n_tables; ++i) {       // every check first: a refusal leaves the slot as it was
        if (int rc = table_device(tables[i], &th[i], &d->tab_sens[i])) return rc;
        d->tab_cons[i] = tables[i].n_points;
        for (int q = 0; q < i; ++q)
            if (d->tab_cons[q] == d->tab_cons[i]) return fail(CSDR_EINVAL, "tables %d and %d both hold %d points: \"cons\" could not tell them apart", q, i, d->tab_cons[i]);
    }
    d->p = csdr_digital_params{};
    d->p.kind = CSDR_DIGITAL_TABLE; d->p.cons = d->tab_cons[0];
    d->g.scheme = DIG_TABLE; d->idx = 0; d->sens = d->tab_sens[0];
    csdr_demod_params q = *p;
    q.bandwidth = p->bandwidth < 500 ? 500 : p->bandwidth;               // ModemDigital.cpp:21-26
    if (int rc = bank_configure_slot(b, slot, &q, post)) return rc;      // (resets the slot, its digital stage included)
    SlotHost &s = b->slots[slot];
    d->cap_sym = s.cfg.cap_iq;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_sym = carve((size_t)d->cap_sym * sizeof(uint32_t)), o_bevm = carve((size_t)b->max_blocks * sizeof(float));
    const size_t o_st = carve((size_t)kDigRecords * 2 * kDigStateFloats * sizeof(float)), o_tab = carve((size_t)n_tables * sizeof(TableDev));
    if (hipMalloc(&d->mem, off) != hipSuccess) { d->mem = nullptr; s.configured = false; return fail(CSDR_ENOMEM, "table slot of %zu bytes", off); }
    char *base = (char *)d->mem;
    d->sym = (uint32_t *)(base + o_sym); d->bevm = (float *)(base + o_bevm); d->st = (float *)(base + o_st); d->tab_d = (TableDev *)(base + o_tab);
    // modemcf_create: r = x_hat = 0 (EVM 0) in every object.  A failure leaves the slot unconfigured.
    if (hipMemset(d->mem, 0, off) != hipSuccess || hipMemcpy(d->tab_d, th.data(), th.size() * sizeof(TableDev), hipMemcpyHostToDevice) != hipSuccess) {
        s.configured = false;
        return fail(CSDR_EHIP, "table slot initialisation: %s", hipGetErrorString(hipGetLastError()));
    }
    s.dig = d;
    return CSDR_OK;
}

extern "C" int csdr_bank_set_digital_cons(csdr_bank *b, int slot, int cons) {
    if (!b || slot < 0 || slot >= b->max_demods || !b->slots[slot].configured || !b->slots[slot].dig) return fail(CSDR_EINVAL, "not a digital slot");
    DigSlot &d = *b->slots[slot].dig;
    const int kind = d.p.kind;
    if (kind == CSDR_DIGITAL_TABLE) {          // a pointer move among the objects created up front
        for (size_t i = 0; i < d.tab_cons.size(); ++i)
            if (d.tab_cons[i] == cons) { d.idx = (int)i; d.p.cons = cons; d.sens = d.tab_sens[i]; return CSDR_OK; }
        return fail(CSDR_EUNSUPPORTED, "cons %d: the slot holds no table of that size", cons);
    }
    if (kind != CSDR_DIGITAL_PSK && kind != CSDR_DIGITAL_DPSK && kind != CSDR_DIGITAL_ASK && kind != CSDR_DIGITAL_QAM)
        return fail(CSDR_EINVAL, "this modem has no \"cons\" setting");
    csdr_digital_params np = d.p;
    np.cons = cons;
    DigGeom g;
    int idx;
    float sens;
    if (int rc = dig_geometry(np, &g, &idx, &sens)) return rc;
    d.p = np; d.g = g; d.idx = idx; d.sens = sens;
    return CSDR_OK;
}

// ModemGMSK::demodulate (ModemGMSK.cpp:116-134) per block of n samples with c = inputBuffer.size() before it: S = c + n, the loop i = 0, k, 2k ..
// < S / k runs I = ceil((S / k) / k) symbols, symbol j reads the block's samples [j k, j k + k) -- past its end: zero here -- and afterwards
// c = S - I k.  No blocks planned (a skipped slot): no demodulate call, nothing changes.
static void gmsk_plan(DigSlot &d, int NB, const BlockPlan *pl) {
    const int k = d.gk;
    d.gblk.assign((size_t)NB + 1, GmskBlock{});
    int32_t off = d.gL - 1, prev = -2, nsym = 0;
    int64_t c = d.gcarry;
    for (int bb = 0; bb < NB; ++bb) {
        csdr_digital_result &r = d.res[bb];
        r.cons = 2;
        const int a = pl ? pl[bb].j0 : 0, n = pl ? pl[bb + 1].j0 - a : 0;
        int64_t I = 0;
        if (pl) {
            const int64_t S = c + n, i_max = S / k;
            I = (i_max + k - 1) / k;
            c = S - I * k;
        }
        r.n_symbols = (int)I; r.symbol_offset = nsym; r.carry = (int32_t)c;
        d.gblk[bb] = GmskBlock{off, a, n, prev};
        if (I > 0) { const int64_t last = I * k - 1; prev = last < n ? a + (int32_t)last : -1; }
        off += (int32_t)(I * k); nsym += (int)I;
    }
    d.gblk[NB] = GmskBlock{off, 0, 0, prev};
    d.nsym_plan = nsym;
    d.gcarry_new = c;
}

void bank_digital_plan(csdr_bank *b, int slot, int NB, const BlockPlan *pl) {
    DigSlot &d = *b->slots[slot].dig;
    d.res.assign((size_t)NB, csdr_digital_result{});
    d.n = pl ? pl[NB].j0 : 0;
    d.run_idx = d.idx; d.run_cons = dig_cons_of(d);
    const bool fsk = d.p.kind == CSDR_DIGITAL_FSK;
    if (d.p.kind == CSDR_DIGITAL_GMSK) { gmsk_plan(d, NB, pl); if (pl) b->dig_run.push_back(slot); else { d.ran = false; d.nsym = 0; } return; }
    for (int bb = 0; bb < NB; ++bb) {
        csdr_digital_result &r = d.res[bb];
        r.cons = d.run_cons;
        const int a = pl ? pl[bb].j0 : 0, e = pl ? pl[bb + 1].j0 : 0;
        if (fsk) {      // the stream the symbols are cut from: the carried samples, then this batch's
            const int64_t sa = (int64_t)d.carry + a, se = (int64_t)d.carry + e;
            r.n_symbols = (int)(se / d.k - sa / d.k); r.symbol_offset = (int)(sa / d.k); r.carry = (int)(se % d.k);
        } else {
            r.n_symbols = e - a; r.symbol_offset = a;
        }
    }
    if (fsk) { const int64_t tot = (int64_t)d.carry + d.n; d.nsym_plan = (int)(tot / d.k); d.new_carry = (int)(tot % d.k); }
    else d.nsym_plan = d.n;
    if (pl) b->dig_run.push_back(slot);
    else { d.ran = false; d.nsym = 0; }
}

// the GMSK slots of the batch: gmsk_phase, then gmsk_decide, on the audio lane behind the front-end
static int gmsk_launch(csdr_bank *b, const std::vector<int> &slots) {
    if (slots.empty()) return CSDR_OK;
    csdr_ctx *c = b->ctx;
    const int nj = (int)slots.size();
    std::vector<GmskJob> &jh = b->gmsk_jobs_h;
    jh.assign((size_t)nj, GmskJob{});
    int gx_phase = 1, gx_decide = 1;
    for (int i = 0; i < nj; ++i) {           // every check first: a refusal leaves every slot as it was
        const DigSlot &d = *b->slots[slots[i]].dig;
        const int nb = (int)d.gblk.size() - 1;
        if (nb > b->max_blocks || d.gblk[nb].off > d.cap_phi || d.nsym_plan > d.cap_sym)
            return fail(CSDR_ERANGE, "GMSK slot %d: %d phase differences / %d symbols exceed its buffers", slots[i], d.gblk[nb].off, d.nsym_plan);
    }
    if (int rc = b->gmsk_jobs.reserve((size_t)b->max_demods)) return rc;
    for (int i = 0; i < nj; ++i) {
        SlotHost &s = b->slots[slots[i]];
        DigSlot &d = *s.dig;
        const int nb = (int)d.gblk.size() - 1;
        const int n_stream = d.gblk[nb].off;
        GmskJob &j = jh[i];
        j.iq = s.cfg.iq + (size_t)s.last_parity * ((size_t)kIqHist + s.cfg.cap_iq) + kIqHist;     // the batch's resampled IQ (csdr_bank_fetch_iq)
        j.blk = d.gblk_d; j.nb = nb; j.L = d.gL; j.k = d.gk; j.nsym = d.nsym_plan; j.h = d.gh;
        j.hist_rd = d.ghist + (size_t)d.hist_cur * (d.gL + 1); j.hist_wr = d.ghist + (size_t)(d.hist_cur ^ 1) * (d.gL + 1);
        j.phi = d.gphi; j.sym = d.sym; j.soft = nullptr;
        gx_phase = std::max(gx_phase, (n_stream + kGmskThreads - 1) / kGmskThreads);
        gx_decide = std::max(gx_decide, (d.nsym_plan + kGmskThreads / 64 - 1) / (kGmskThreads / 64));
        CSDR_HIP_TRY(hipMemcpyAsync(d.gblk_d, d.gblk.data(), d.gblk.size() * sizeof(GmskBlock), hipMemcpyHostToDevice, c->lanes[LANE_AUDIO]));
        d.hist_cur ^= 1; d.gcarry = d.gcarry_new; d.nsym = d.nsym_plan; d.ran = true;
    }
    CSDR_HIP_TRY(hipMemcpyAsync(b->gmsk_jobs.p, jh.data(), (size_t)nj * sizeof(GmskJob), hipMemcpyHostToDevice, c->lanes[LANE_AUDIO]));
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, gmsk_phase, dim3(gx_phase, nj), dim3(kGmskThreads), 0, (const GmskJob *)b->gmsk_jobs.p);
    CSDR_HIP_TRY(hipGetLastError());
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, gmsk_decide, dim3(gx_decide, nj), dim3(kGmskThreads), 0, (const GmskJob *)b->gmsk_jobs.p);
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

// the table slots of the batch: one table_demod launch, on the audio lane behind the front-end
static int table_launch(csdr_bank *b, const std::vector<int> &slots, const BlockPlan *plans_d, int NB) {
    if (slots.empty()) return CSDR_OK;
    csdr_ctx *c = b->ctx;
    const int nj = (int)slots.size();
    if (int rc = b->tab_jobs.reserve((size_t)b->max_demods)) return rc;
    std::vector<TableJob> &jh = b->tab_jobs_h;
    jh.assign((size_t)nj, TableJob{});
    int gx = 1;
    for (int i = 0; i < nj; ++i) {
        const int si = slots[i];
        SlotHost &s = b->slots[si];
        DigSlot &d = *s.dig;
        TableJob &j = jh[i];
        j.iq = s.cfg.iq + (size_t)s.last_parity * ((size_t)kIqHist + s.cfg.cap_iq) + kIqHist;     // the batch's resampled IQ (csdr_bank_fetch_iq)
        j.n = std::min(d.n, d.cap_sym); j.nb = NB; j.plan = plans_d + (size_t)si * (NB + 1);
        j.sym = d.sym; j.bevm = d.bevm; j.tab = d.tab_d + d.idx;
        j.st_rd = d.st + (size_t)(2 * d.idx + d.st_cur[d.idx]) * kDigStateFloats;
        j.st_wr = d.st + (size_t)(2 * d.idx + (d.st_cur[d.idx] ^ 1)) * kDigStateFloats;
        gx = std::max(gx, (j.n + kTabThreads - 1) / kTabThreads);
        if (d.n > 0) d.st_cur[d.idx] ^= 1;
        d.nsym = d.nsym_plan; d.ran = true;
    }
    CSDR_HIP_TRY(hipMemcpyAsync(b->tab_jobs.p, jh.data(), (size_t)nj * sizeof(TableJob), hipMemcpyHostToDevice, c->lanes[LANE_AUDIO]));
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, table_demod, dim3(gx, nj), dim3(kTabThreads), sizeof(TableDev), (const TableJob *)b->tab_jobs.p);
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

int bank_digital_launch(csdr_bank *b, const BlockPlan *plans_d, int NB) {
    if (b->dig_run.empty()) return CSDR_OK;
    csdr_ctx *c = b->ctx;
    std::vector<int> run, gmsk, table;
    for (int si : b->dig_run) {
        const int kind = b->slots[si].dig->p.kind;
        (kind == CSDR_DIGITAL_GMSK ? gmsk : kind == CSDR_DIGITAL_TABLE ? table : run).push_back(si);
    }
    if (int rc = gmsk_launch(b, gmsk)) return rc;
    if (int rc = table_launch(b, table, plans_d, NB)) return rc;
    if (run.empty()) return CSDR_OK;
    const int nj = (int)run.size();
    if (int rc = b->dig_jobs.reserve((size_t)b->max_demods * sizeof(DigJob))) return rc;
    b->dig_jobs_h.assign((size_t)nj * sizeof(DigJob), 0);
    DigJob *jh = reinterpret_cast<DigJob *>(b->dig_jobs_h.data());
    int gx = 1;
    for (int i = 0; i < nj; ++i) {
        const int si = run[i];
        SlotHost &s = b->slots[si];
        DigSlot &d = *s.dig;
        DigJob &j = jh[i];
        j.iq = s.cfg.iq + (size_t)s.last_parity * ((size_t)kIqHist + s.cfg.cap_iq) + kIqHist;     // the batch's resampled IQ (csdr_bank_fetch_iq)
        j.n = d.n; j.nb = NB; j.plan = plans_d + (size_t)si * (NB + 1);
        j.sym = d.sym; j.bevm = d.bevm; j.g = d.g;
        if (d.p.kind == CSDR_DIGITAL_FSK) {
            j.k = d.k; j.K = d.K; j.M = d.M; j.carry = d.carry; j.nsym = d.nsym_plan; j.new_carry = d.new_carry; j.map = d.map;
            j.stash_rd = d.stash + (size_t)d.stash_cur * kDigFskMaxK; j.stash_wr = d.stash + (size_t)(d.stash_cur ^ 1) * kDigFskMaxK;
            gx = std::max(gx, (d.nsym_plan + kDigThreads / 64 - 1) / (kDigThreads / 64));
            d.carry = d.new_carry; d.stash_cur ^= 1;
        } else {
            j.st_rd = d.st + (size_t)(2 * d.idx + d.st_cur[d.idx]) * kDigStateFloats;
            j.st_wr = d.st + (size_t)(2 * d.idx + (d.st_cur[d.idx] ^ 1)) * kDigStateFloats;
            gx = std::max(gx, (d.n + kDigThreads - 1) / kDigThreads);
            if (d.n > 0) d.st_cur[d.idx] ^= 1;
        }
        d.nsym = d.nsym_plan; d.ran = true;
    }
    CSDR_HIP_TRY(hipMemcpyAsync(b->dig_jobs.p, jh, (size_t)nj * sizeof(DigJob), hipMemcpyHostToDevice, c->lanes[LANE_AUDIO]));
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, digital_demod, dim3(gx, nj), dim3(kDigThreads), 0, reinterpret_cast<const DigJob *>(b->dig_jobs.p));
    CSDR_HIP_TRY(hipGetLastError());
    return CSDR_OK;
}

extern "C" int csdr_bank_fetch_digital_results(csdr_bank *b, int slot, csdr_digital_result *out, int cap_blocks, int *n_blocks) {
    DeviceScope dev__(b ? b->ctx : nullptr);
    if (!b || !out || !n_blocks || slot < 0 || slot >= b->max_demods) return fail(CSDR_EINVAL, "bad argument");
    SlotHost &s = b->slots[slot];
    if (!s.configured || !s.dig) return fail(CSDR_EINVAL, "slot %d is not a digital slot", slot);
    DigSlot &d = *s.dig;
    const int nb = (int)d.res.size();
    if (nb > cap_blocks) return fail(CSDR_ERANGE, "need room for %d blocks", nb);
    *n_blocks = nb;
    if (!nb) return CSDR_OK;
    if (d.sens >= 0.0f) {
        std::vector<float> evm((size_t)nb);
        hipStream_t st = b->ctx->lanes[LANE_AUDIO];
        if (d.ran) CSDR_HIP_TRY(hipMemcpyAsync(evm.data(), d.bevm, (size_t)nb * sizeof(float), hipMemcpyDeviceToHost, st));
        else {      // skipped batch: the object still holds the state of the one before
            float rec[kDigStateFloats];
            CSDR_HIP_TRY(hipMemcpyAsync(rec, d.st + (size_t)(2 * d.run_idx + d.st_cur[d.run_idx]) * kDigStateFloats, sizeof rec, hipMemcpyDeviceToHost, st));
            CSDR_HIP_TRY(hipStreamSynchronize(st));
            std::fill(evm.begin(), evm.end(), dig_evm(make_float2(rec[0], rec[1]), make_float2(rec[2], rec[3])));
        }
        CSDR_HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < nb; ++i) { d.res[i].evm = evm[i]; d.res[i].lock = evm[i] <= d.sens; }
    }
    memcpy(out, d.res.data(), (size_t)nb * sizeof(csdr_digital_result));
    return CSDR_OK;
}

extern "C" int csdr_bank_fetch_symbols(csdr_bank *b, int slot, uint32_t *host_out, int cap, int *n) {
    DeviceScope dev__(b ? b->ctx : nullptr);
    if (!b || !n || slot < 0 || slot >= b->max_demods) return fail(CSDR_EINVAL, "bad argument");
    SlotHost &s = b->slots[slot];
    if (!s.configured || !s.dig) return fail(CSDR_EINVAL, "slot %d is not a digital slot", slot);
    DigSlot &d = *s.dig;
    const int cnt = d.ran ? d.nsym : 0;
    if (cnt > cap) return fail(CSDR_ERANGE, "need room for %d symbols", cnt);
    if (cnt && !host_out) return fail(CSDR_EINVAL, "null output");
    *n = cnt;
    if (cnt) {
        hipStream_t st = b->ctx->lanes[LANE_AUDIO];
        CSDR_HIP_TRY(hipMemcpyAsync(host_out, d.sym, (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CSDR_HIP_TRY(hipStreamSynchronize(st));
    }
    return CSDR_OK;
}

extern "C" int csdr_digital_run(csdr_ctx *c, const csdr_digital_params *dp, int64_t sample_rate, const float *iq_host, int n, csdr_digital_state *state,
                                uint32_t *sym_host, int cap_symbols, int *n_symbols, float *evm_last) {
    DeviceScope dev__(c);
    if (!c || !dp || !state || !n_symbols || n < 0 || (n > 0 && !iq_host) || sample_rate <= 0) return fail(CSDR_EINVAL, "bad argument");
    DigSlot d;
    std::vector<uint32_t> map;
    if (int rc = dig_setup(dp, sample_rate, &d, &map)) return rc;
    const bool fsk = d.p.kind == CSDR_DIGITAL_FSK;
    if (fsk && (state->n_carry < 0 || state->n_carry >= d.k)) return fail(CSDR_EINVAL, "state holds %d carried samples, k = %d", state->n_carry, d.k);
    const int carry = fsk ? state->n_carry : 0;
    const int nsym = fsk ? (int)(((int64_t)carry + n) / d.k) : n, new_carry = fsk ? (int)(((int64_t)carry + n) % d.k) : 0;
    if (nsym > cap_symbols || (nsym > 0 && !sym_host)) return fail(CSDR_ERANGE, "need room for %d symbols", nsym);
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_job = carve(sizeof(DigJob)), o_plan = carve(2 * sizeof(BlockPlan)), o_bevm = carve(sizeof(float)),
                 o_st = carve(2 * kDigStateFloats * sizeof(float)), o_iq = carve(std::max(1, n) * sizeof(float2)),
                 o_sym = carve(std::max(1, nsym) * sizeof(uint32_t)), o_stash = carve((size_t)2 * kDigFskMaxK * sizeof(float2)),
                 o_map = carve(std::max<size_t>(1, map.size()) * sizeof(uint32_t));
    void *mem = nullptr;
    if (hipMalloc(&mem, off) != hipSuccess) return fail(CSDR_ENOMEM, "%zu bytes", off);
    std::unique_ptr<void, void (*)(void *)> guard(mem, [](void *p) { (void)hipFree(p); });
    char *base = (char *)mem;
    hipStream_t st = c->lanes[LANE_AUDIO];
    const BlockPlan plan[2] = {{0, 0}, {n, n}};
    float rec[2 * kDigStateFloats] = {state->r[0], state->r[1], state->x_hat[0], state->x_hat[1], state->phi};
    DigJob j;
    memset(&j, 0, sizeof j);
    j.iq = (const float2 *)(base + o_iq); j.n = n; j.nb = 1; j.plan = (const BlockPlan *)(base + o_plan);
    j.sym = (uint32_t *)(base + o_sym); j.bevm = (float *)(base + o_bevm);
    j.st_rd = (const float *)(base + o_st); j.st_wr = (float *)(base + o_st) + kDigStateFloats; j.g = d.g;
    j.k = d.k; j.K = d.K; j.M = d.M; j.carry = carry; j.nsym = fsk ? nsym : 0; j.new_carry = new_carry; j.map = (const uint32_t *)(base + o_map);
    j.stash_rd = (const float2 *)(base + o_stash); j.stash_wr = (float2 *)(base + o_stash) + kDigFskMaxK;
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_job, &j, sizeof j, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_plan, plan, sizeof plan, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_st, rec, sizeof rec, hipMemcpyHostToDevice, st));
    if (n) CSDR_HIP_TRY(hipMemcpyAsync(base + o_iq, iq_host, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    if (carry) CSDR_HIP_TRY(hipMemcpyAsync(base + o_stash, state->carry, (size_t)carry * sizeof(float2), hipMemcpyHostToDevice, st));
    if (!map.empty()) CSDR_HIP_TRY(hipMemcpyAsync(base + o_map, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const int gx = std::max(1, fsk ? (nsym + kDigThreads / 64 - 1) / (kDigThreads / 64) : (n + kDigThreads - 1) / kDigThreads);
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, digital_demod, dim3(gx, 1), dim3(kDigThreads), 0, reinterpret_cast<const DigJob *>(base + o_job));
    CSDR_HIP_TRY(hipGetLastError());
    float evm = 0.0f;
    if (nsym) CSDR_HIP_TRY(hipMemcpyAsync(sym_host, base + o_sym, (size_t)nsym * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipMemcpyAsync(rec, base + o_st, sizeof rec, hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipMemcpyAsync(&evm, base + o_bevm, sizeof evm, hipMemcpyDeviceToHost, st));
    std::vector<float2> stash_out((size_t)std::max(1, new_carry));
    if (new_carry) CSDR_HIP_TRY(hipMemcpyAsync(stash_out.data(), base + o_stash + (size_t)kDigFskMaxK * sizeof(float2), (size_t)new_carry * sizeof(float2), hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipStreamSynchronize(st));
    if (fsk) {
        state->n_carry = new_carry;
        memcpy(state->carry, stash_out.data(), (size_t)new_carry * sizeof(float2));
        evm = 0.0f;
    } else if (n > 0) {
        const float *w = rec + kDigStateFloats;
        state->r[0] = w[0]; state->r[1] = w[1]; state->x_hat[0] = w[2]; state->x_hat[1] = w[3]; state->phi = w[4];
    }
    *n_symbols = nsym;
    if (evm_last) *evm_last = evm;
    return CSDR_OK;
}

extern "C" int csdr_table_run(csdr_ctx *c, const csdr_constellation *table, const float *iq_host, int n, csdr_digital_state *state,
                              uint32_t *sym_host, int cap_symbols, int *n_symbols, float *evm_last) {
    DeviceScope dev__(c);
    if (!c || !table || !state || !n_symbols || n < 0 || (n > 0 && !iq_host)) return fail(CSDR_EINVAL, "bad argument");
    TableDev th;
    float sens;
    if (int rc = table_device(*table, &th, &sens)) return rc;
    if (n > cap_symbols || (n > 0 && !sym_host)) return fail(CSDR_ERANGE, "need room for %d symbols", n);
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_job = carve(sizeof(TableJob)), o_plan = carve(2 * sizeof(BlockPlan)), o_bevm = carve(sizeof(float)),
                 o_st = carve(2 * kDigStateFloats * sizeof(float)), o_iq = carve((size_t)std::max(1, n) * sizeof(float2)),
                 o_sym = carve((size_t)std::max(1, n) * sizeof(uint32_t)), o_tab = carve(sizeof(TableDev));
    void *mem = nullptr;
    if (hipMalloc(&mem, off) != hipSuccess) return fail(CSDR_ENOMEM, "%zu bytes", off);
    std::unique_ptr<void, void (*)(void *)> guard(mem, [](void *p) { (void)hipFree(p); });
    char *base = (char *)mem;
    hipStream_t st = c->lanes[LANE_AUDIO];
    const BlockPlan plan[2] = {{0, 0}, {n, n}};
    float rec[2 * kDigStateFloats] = {state->r[0], state->r[1], state->x_hat[0], state->x_hat[1]};
    TableJob j{};
    j.iq = (const float2 *)(base + o_iq); j.n = n; j.nb = 1; j.plan = (const BlockPlan *)(base + o_plan);
    j.sym = (uint32_t *)(base + o_sym); j.bevm = (float *)(base + o_bevm);
    j.st_rd = (const float *)(base + o_st); j.st_wr = (float *)(base + o_st) + kDigStateFloats; j.tab = (const TableDev *)(base + o_tab);
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_job, &j, sizeof j, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_plan, plan, sizeof plan, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_st, rec, sizeof rec, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_tab, &th, sizeof th, hipMemcpyHostToDevice, st));
    if (n) CSDR_HIP_TRY(hipMemcpyAsync(base + o_iq, iq_host, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    const int gx = std::max(1, (n + kTabThreads - 1) / kTabThreads);
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, table_demod, dim3(gx, 1), dim3(kTabThreads), sizeof(TableDev), (const TableJob *)(base + o_job));
    CSDR_HIP_TRY(hipGetLastError());
    float evm = 0.0f;
    if (n) CSDR_HIP_TRY(hipMemcpyAsync(sym_host, base + o_sym, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipMemcpyAsync(rec, base + o_st, sizeof rec, hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipMemcpyAsync(&evm, base + o_bevm, sizeof evm, hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipStreamSynchronize(st));
    if (n > 0) {
        const float *w = rec + kDigStateFloats;
        state->r[0] = w[0]; state->r[1] = w[1]; state->x_hat[0] = w[2]; state->x_hat[1] = w[3];
    }
    *n_symbols = n;
    if (evm_last) *evm_last = evm;
    return CSDR_OK;
}

extern "C" int csdr_gmsk_run(csdr_ctx *c, const csdr_digital_params *dp, const float *iq_host, int n, csdr_gmsk_state *state, float *history,
                             uint32_t *sym_host, float *soft_host, int cap_symbols, int *n_symbols) {
    DeviceScope dev__(c);
    if (!c || !dp || !state || !history || !n_symbols || n < 0 || (n > 0 && !iq_host)) return fail(CSDR_EINVAL, "bad argument");
    if (dp->kind != CSDR_DIGITAL_GMSK) return fail(CSDR_EINVAL, "csdr_gmsk_run: kind must be CSDR_DIGITAL_GMSK");
    DigSlot d;
    std::vector<uint32_t> map;
    if (int rc = dig_setup(dp, 500, &d, &map)) return rc;
    const int k = d.gk, L = d.gL;
    if (n % k) return fail(CSDR_EINVAL, "csdr_gmsk_run: %d samples are not whole symbols of %d", n, k);
    const int nsym = n / k;
    if (nsym > cap_symbols || (nsym > 0 && !sym_host)) return fail(CSDR_ERANGE, "need room for %d symbols", nsym);
    const std::vector<float> taps = design::gmsk_rx_taps((unsigned)k, (unsigned)d.gm, d.p.bw);
    const GmskBlock blk[2] = {{L - 1, 0, n, -2}, {L - 1 + n, 0, 0, n > 0 ? n - 1 : -2}};
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_job = carve(sizeof(GmskJob)), o_blk = carve(sizeof blk), o_h = carve((size_t)L * sizeof(float)),
                 o_hist = carve((size_t)2 * (L + 1) * sizeof(float)), o_iq = carve((size_t)std::max(1, n) * sizeof(float2)),
                 o_phi = carve((size_t)(L - 1 + n) * sizeof(float)), o_sym = carve((size_t)std::max(1, nsym) * sizeof(uint32_t)),
                 o_soft = carve((size_t)std::max(1, nsym) * sizeof(float));
    void *mem = nullptr;
    if (hipMalloc(&mem, off) != hipSuccess) return fail(CSDR_ENOMEM, "%zu bytes", off);
    std::unique_ptr<void, void (*)(void *)> guard(mem, [](void *p) { (void)hipFree(p); });
    char *base = (char *)mem;
    hipStream_t st = c->lanes[LANE_AUDIO];
    std::vector<float> hist((size_t)L + 1);
    memcpy(hist.data(), history, (size_t)(L - 1) * sizeof(float));
    hist[L - 1] = state->x_prime[0]; hist[L] = state->x_prime[1];
    GmskJob j{};
    j.iq = (const float2 *)(base + o_iq); j.blk = (const GmskBlock *)(base + o_blk); j.nb = 1; j.L = L; j.k = k; j.nsym = nsym;
    j.h = (const float *)(base + o_h); j.hist_rd = (const float *)(base + o_hist); j.hist_wr = (float *)(base + o_hist) + (L + 1);
    j.phi = (float *)(base + o_phi); j.sym = (uint32_t *)(base + o_sym); j.soft = (float *)(base + o_soft);
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_job, &j, sizeof j, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_blk, blk, sizeof blk, hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_h, taps.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice, st));
    CSDR_HIP_TRY(hipMemcpyAsync(base + o_hist, hist.data(), hist.size() * sizeof(float), hipMemcpyHostToDevice, st));
    if (n) CSDR_HIP_TRY(hipMemcpyAsync(base + o_iq, iq_host, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    const int gx_phase = (L - 1 + n + kGmskThreads - 1) / kGmskThreads, gx_decide = std::max(1, (nsym + kGmskThreads / 64 - 1) / (kGmskThreads / 64));
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, gmsk_phase, dim3(gx_phase, 1), dim3(kGmskThreads), 0, (const GmskJob *)(base + o_job));
    CSDR_HIP_TRY(hipGetLastError());
    CSDR_LAUNCH(c, LANE_AUDIO, KID_DIGITAL, gmsk_decide, dim3(gx_decide, 1), dim3(kGmskThreads), 0, (const GmskJob *)(base + o_job));
    CSDR_HIP_TRY(hipGetLastError());
    if (nsym) {
        CSDR_HIP_TRY(hipMemcpyAsync(sym_host, base + o_sym, (size_t)nsym * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (soft_host) CSDR_HIP_TRY(hipMemcpyAsync(soft_host, base + o_soft, (size_t)nsym * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    CSDR_HIP_TRY(hipMemcpyAsync(hist.data(), base + o_hist + (size_t)(L + 1) * sizeof(float), hist.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    CSDR_HIP_TRY(hipStreamSynchronize(st));
    memcpy(history, hist.data(), (size_t)(L - 1) * sizeof(float));
    state->x_prime[0] = hist[L - 1]; state->x_prime[1] = hist[L];
    *n_symbols = nsym;
    return CSDR_OK;
}
