// match.cpp -- host side of the template-correlation accumulator (include/iqgpu.h "template correlation"; kernels match.hip; DESIGN
// 3.14): the options, the row arithmetic, the template spectra G_t, the shift bank and the detections (no device), and the
// iqgpu_match handle -- the stream core and the open row's record per template in two buffers -- with push / push_device / read_open /
// reset.  Independent of any chain.  Segment grid, stream position, carry, twiddles and streams are the power spectrum's: PsdStream
// (psd.hpp, psd.cpp), opened with hop = nfft / 2, a rectangular window and gain 1.
#include "chain.hpp"
#include "match.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr size_t kPushSliceFrames = (size_t)1 << 20;     // of a host push: frames staged per slice (its rows come back per slice)
constexpr uint32_t kMaxBlockFrames = (uint32_t)1 << 24;
const char *const kReset = "iqgpu_match_reset";

// nfft as the kernels run it: the option, or for 0 the smallest of the three sizes that holds the template
uint32_t nfft_of(const iqgpu_match_opts &o)
{
    if (o.nfft) return o.nfft;
    for (uint32_t n = 1024; n <= 4096; n *= 2)
        if (n / 2 + 1 >= o.template_frames) return n;
    return 0;
}

// o's part that is the power spectrum's
iqgpu_psd_opts psd_part(const iqgpu_match_opts &o)
{
    iqgpu_psd_opts q{};
    q.nfft = nfft_of(o); q.hop = q.nfft / 2; q.window = IQGPU_PSD_RECT; q.gain = 1.0f;
    return q;
}

int check_opts(const iqgpu_match_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (o->nfft != 0 && o->nfft != 1024 && o->nfft != 2048 && o->nfft != 4096) return fail(IQGPU_EINVAL, "%s: nfft %u is not 0, 1024, 2048 or 4096", who, o->nfft);
    if (o->n_templates < 1 || o->n_templates > (uint32_t)kMatchMaxTemplates)
        return fail(IQGPU_EINVAL, "%s: n_templates %u is not in 1 .. %d", who, o->n_templates, kMatchMaxTemplates);
    const uint32_t nfft = nfft_of(*o);
    if (o->template_frames < 2 || !nfft || o->template_frames > nfft / 2 + 1)
        return fail(IQGPU_EINVAL, "%s: template_frames %u is not in 2 .. %u", who, o->template_frames, nfft ? nfft / 2 + 1 : 2049u);
    const uint32_t B = o->block_frames;
    if (B < nfft / 2 || B > kMaxBlockFrames || (B & (B - 1)) != 0)
        return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in %u .. %u", who, B, nfft / 2, kMaxBlockFrames);
    return IQGPU_OK;
}

uint64_t rows_of(const iqgpu_match_opts &o, uint64_t frames)
{
    const iqgpu_psd_opts q = psd_part(o);
    return psd_segments_of(q, frames) / (o.block_frames / q.hop);
}

// G_t[k] = conj(sum_n h_t[n] exp(-2 pi i k n / nfft)) / nfft for every template, and the templates' energies: double, rounded once
int fill_spectra(const iqgpu_match_opts &o, const float *tmpl, std::vector<float> &g, double *energy, const char *who)
{
    const uint32_t N = nfft_of(o), L = o.template_frames;
    std::vector<double> tw;
    try { tw.resize(2 * (size_t)N); g.resize(2 * (size_t)N * o.n_templates); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "%s: out of host memory", who); }
    for (uint32_t k = 0; k < N; ++k) {
        const double a = 2.0 * kPi * (double)k / (double)N;
        tw[2 * k] = std::cos(a); tw[2 * k + 1] = std::sin(a);
    }
    for (uint32_t t = 0; t < o.n_templates; ++t) {
        const float *h = tmpl + 2 * (size_t)t * L;
        double e = 0.0;
        for (uint32_t n = 0; n < 2 * L; ++n) {
            if (!std::isfinite(h[n])) return fail(IQGPU_EINVAL, "%s: template %u holds a value that is not finite", who, t);
            e += (double)h[n] * (double)h[n];
        }
        if (!(e > 0.0)) return fail(IQGPU_EINVAL, "%s: template %u has no energy", who, t);
        energy[t] = e;
        float *gt = g.data() + 2 * (size_t)t * N;
        for (uint32_t k = 0; k < N; ++k) {
            // conj(h exp(-i a)) = conj(h) exp(+i a)
            double re = 0.0, im = 0.0;
            for (uint32_t n = 0; n < L; ++n) {
                const uint32_t at = (uint32_t)(((uint64_t)k * n) & (N - 1));
                const double c = tw[2 * at], s = tw[2 * at + 1], hr = h[2 * n], hi = h[2 * n + 1];
                re += hr * c + hi * s;
                im += hr * s - hi * c;
            }
            gt[2 * k] = (float)(re / (double)N); gt[2 * k + 1] = (float)(im / (double)N);
        }
    }
    return IQGPU_OK;
}

} // namespace

struct iqgpu_match {
    PsdStream st;
    iqgpu_match_opts o{};                 // nfft resolved
    double energy[kMatchMaxTemplates] = {};
    int open_cur = 0;                     // which half of `open` holds the open row (a launch writes the other: match.hip)
    DevBuf g, open, slab, rows_out;
    size_t slab_segs = 0;
    int64_t V() const { return (int64_t)o.nfft / 2; }
    int64_t R() const { return (int64_t)o.block_frames / V(); }
    MatchRec *open_rec(int i) const { return (MatchRec *)open.p + (size_t)i * kMatchMaxTemplates; }
    size_t open_bytes() const { return 2 * (size_t)kMatchMaxTemplates * sizeof(MatchRec); }
    uint64_t rows_after(size_t n) const { return psd_segments_of(st.q, st.frames + n) / (uint64_t)R(); }
    IQGPU_LOCAL ~iqgpu_match() { st.close(); }        // the waits first: the members free themselves behind them
};

namespace {

PsdStream *core(iqgpu_match *p) { return p ? &p->st : nullptr; }

// n frames of device memory behind everything pushed so far, on s; the rows they complete into the three device planes (any may be NULL)
int push_frames(iqgpu_match *p, const void *d_raw, size_t n, float *d_peak, uint32_t *d_at, float *d_sum, hipStream_t s)
{
    PsdStream &st = p->st;
    PsdPush u;
    int rc = st.enter(d_raw, n, s, &u); if (rc) return rc;
    const int64_t R = p->R(), nt = p->o.n_templates, m = u.m, cap = kMatchSlabSegments;
    if (m > 0) {                                                                  // the slab: sized before anything is queued (psd.cpp on growing such a buffer)
        const size_t segs = (size_t)(m < cap ? m : cap);
        if (segs > p->slab_segs) {
            rc = p->slab.ensure(segs * (size_t)nt * sizeof(MatchRec)); if (rc) return rc;
            p->slab_segs = segs;
        }
    }
    st.poisoned = true;                                                           // (until finish() has queued the last of the push)
    for (int64_t j = 0; j < m;) {
        const int64_t seg0 = (int64_t)st.segments + j, cnt = m - j < cap ? m - j : cap, seg_end = seg0 + cnt, r0 = seg0 / R;
        MatchSegsArgs a{};
        st.fill(u, j, cnt, &a);
        a.g = (const cf2 *)p->g.p; a.n_templates = (int32_t)nt; a.slab = (MatchRec *)p->slab.p;
        HIP_TRY(launch_match_segs(a, s));
        MatchFoldArgs f{};
        f.slab = a.slab; f.n_templates = (int32_t)nt; f.n_rows = (int32_t)((seg_end - 1) / R - r0 + 1); f.has_open_in = seg0 % R != 0; f.V = (int32_t)p->V();
        f.R = R; f.r0 = r0; f.seg0 = seg0; f.seg_end = seg_end;
        f.open_in = p->open_rec(p->open_cur); f.open_out = p->open_rec(p->open_cur ^ 1);
        f.row_peak = d_peak; f.row_at = d_at; f.row_sum = d_sum;
        HIP_TRY(launch_match_fold(f, s));
        p->open_cur ^= 1;                                                         // the open row, if the launch left one, is in the other half
        const int64_t done = seg_end / R - r0;                                    // rows the launch finished
        if (d_peak) d_peak += done * nt;
        if (d_at) d_at += done * nt;
        if (d_sum) d_sum += done * nt;
        j += cnt;
    }
    return st.finish(u);
}

// the checks of both pushes, in front of anything queued; *need = the rows the push completes
int begin_push(iqgpu_match *p, const void *raw, size_t frames, bool planes, size_t cap_rows, size_t *rows, size_t *need, const char *who)
{
    if (rows) *rows = 0;
    const int rc = PsdStream::guard(core(p), raw || !frames, who, kReset, false); if (rc) return rc;
    *need = (size_t)(p->rows_after(frames) - p->st.segments / (uint64_t)p->R());
    if (planes && *need > cap_rows)
        return fail(IQGPU_ECAPACITY, "%s: room for %zu rows, the push completes %zu (iqgpu_match_max_rows)", who, cap_rows, *need);
    if (frames) HIP_TRY(hipSetDevice(p->st.device));
    return IQGPU_OK;
}

} // namespace

extern "C" void iqgpu_match_opts_init(iqgpu_match_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->nfft = 0; o->block_frames = 4096; o->n_templates = 1; o->template_frames = 0;
}

extern "C" int iqgpu_match_rows(const iqgpu_match_opts *o, uint64_t frames, uint64_t *rows)
{
    const int rc = check_opts(o, "iqgpu_match_rows"); if (rc) return rc;
    if (!rows) return fail(IQGPU_EINVAL, "iqgpu_match_rows: NULL argument");
    *rows = rows_of(*o, frames);
    return IQGPU_OK;
}

extern "C" int iqgpu_match_create(int device, int format, const iqgpu_match_opts *o, const float *templates, iqgpu_match **out)
{
    const char *who = "iqgpu_match_create";
    if (out) *out = nullptr;
    if (!out || !templates) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    std::vector<float> gtab;                                         // the sources of the uploads: until the synchronise below
    double energy[kMatchMaxTemplates] = {};
    rc = fill_spectra(*o, templates, gtab, energy, who); if (rc) return rc;
    const iqgpu_psd_opts q = psd_part(*o);
    iqgpu_match *p = new (std::nothrow) iqgpu_match;
    std::vector<float> tab;
    rc = PsdStream::open(core(p), device, format, &q, who, tab);
    if (rc == IQGPU_OK) {
        p->o = *o; p->o.nfft = q.nfft;
        memcpy(p->energy, energy, sizeof(energy));
        rc = p->open.ensure(p->open_bytes());
    }
    if (rc == IQGPU_OK) rc = p->g.ensure(gtab.size() * sizeof(float));
    if (rc == IQGPU_OK) {
        hipError_t e = hipMemcpyAsync(p->g.p, gtab.data(), gtab.size() * sizeof(float), hipMemcpyHostToDevice, p->st.own);
        if (e == hipSuccess) e = hipMemsetAsync(p->open.p, 0, p->open_bytes(), p->st.own);
        if (e == hipSuccess) e = hipStreamSynchronize(p->st.own);
        if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_match_destroy(iqgpu_match *p) { delete p; }

extern "C" int iqgpu_match_reset(iqgpu_match *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_match_reset: NULL argument");
    const int rc = p->st.begin_reset(); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(p->open.p, 0, p->open_bytes(), p->st.own));
    HIP_TRY(hipStreamSynchronize(p->st.own));
    p->st.rewind(); p->open_cur = 0;
    return IQGPU_OK;
}

extern "C" size_t iqgpu_match_max_rows(const iqgpu_match *p, size_t frames)
{
    return p ? (size_t)(p->rows_after(frames) - p->st.segments / (uint64_t)p->R()) : 0;
}

extern "C" int iqgpu_match_push_device(iqgpu_match *p, const void *d_raw, size_t frames, float *d_row_peak, uint32_t *d_row_at, float *d_row_sum,
                                       size_t cap_rows, size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = begin_push(p, d_raw, frames, d_row_peak || d_row_at || d_row_sum, cap_rows, rows, &need, "iqgpu_match_push_device"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_peak, d_row_at, d_row_sum, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_match_push(iqgpu_match *p, const void *raw, size_t frames, float *row_peak, uint32_t *row_at, float *row_sum, size_t cap_rows,
                                size_t *rows)
{
    size_t need = 0;
    int rc = begin_push(p, raw, frames, row_peak || row_at || row_sum, cap_rows, rows, &need, "iqgpu_match_push"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    PsdStream &st = p->st;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames, nt = p->o.n_templates;
    // rows of one slice, whatever the position: the segments that start in a slice, and the one a carry completes
    const size_t slice_rows = (slice / (size_t)p->V() + 1) / (size_t)p->R() + 1, plane = slice_rows * nt * sizeof(float);
    rc = st.stage.ensure(slice * st.bps); if (rc) return rc;
    rc = p->rows_out.ensure(3 * plane); if (rc) return rc;
    float *d_peak = row_peak ? (float *)p->rows_out.p : nullptr;
    uint32_t *d_at = row_at ? (uint32_t *)((char *)p->rows_out.p + plane) : nullptr;
    float *d_sum = row_sum ? (float *)((char *)p->rows_out.p + 2 * plane) : nullptr;
    if (rows) *rows = need;
    HostPlane out[3] = {{(char *)row_peak, d_peak, nt * sizeof(float)}, {(char *)row_at, d_at, nt * sizeof(uint32_t)}, {(char *)row_sum, d_sum, nt * sizeof(float)}};
    return push_host_slices(st, st.stage, raw, frames, kPushSliceFrames, slice_rows, out, "iqgpu_match_push", "completes",
                            [&](size_t n) { return iqgpu_match_max_rows(p, n); },
                            [&](const void *d_raw, size_t n) { return push_frames(p, d_raw, n, d_peak, d_at, d_sum, st.own); });
}

extern "C" int iqgpu_match_read_open(iqgpu_match *p, double *sum, float *peak, uint32_t *at, iqgpu_match_info *info)
{
    int rc = PsdStream::guard(core(p), true, "iqgpu_match_read_open", kReset); if (rc) return rc;
    rc = p->st.settle(); if (rc) return rc;
    const uint32_t nt = p->o.n_templates, open_segments = (uint32_t)(p->st.segments % (uint64_t)p->R());
    if (sum || peak || at) {
        MatchRec rec[kMatchMaxTemplates] = {};                           // what the arithmetic says is empty is not looked at
        if (open_segments) HIP_TRY(hipMemcpy(rec, p->open_rec(p->open_cur), nt * sizeof(MatchRec), hipMemcpyDeviceToHost));
        for (uint32_t t = 0; t < nt; ++t) {
            if (sum) sum[t] = rec[t].sum;
            if (peak) peak[t] = rec[t].peak;
            if (at) at[t] = rec[t].at;
        }
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->frames = p->st.frames; info->segments = p->st.segments; info->rows = p->st.segments / (uint64_t)p->R(); info->open_segments = open_segments;
        info->nfft = p->o.nfft; info->block_frames = p->o.block_frames; info->n_templates = nt; info->template_frames = p->o.template_frames;
        memcpy(info->template_energy, p->energy, sizeof(p->energy));
    }
    return IQGPU_OK;
}

// ---- host only ----
extern "C" int iqgpu_match_shift_bank(const float *tmpl, uint32_t template_frames, const double *hz, uint32_t n, double sample_rate, float *out)
{
    const char *who = "iqgpu_match_shift_bank";
    if (!tmpl || !hz || !out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (template_frames < 1 || n < 1) return fail(IQGPU_EINVAL, "%s: no frames or no members", who);
    if (!(sample_rate > 0.0) || !std::isfinite(sample_rate)) return fail(IQGPU_EINVAL, "%s: sample_rate is not a positive finite number", who);
    for (uint32_t i = 0; i < n; ++i)
        if (!std::isfinite(hz[i])) return fail(IQGPU_EINVAL, "%s: member %u's offset is not finite", who, i);
    for (uint32_t i = 0; i < n; ++i) {
        float *o = out + 2 * (size_t)i * template_frames;
        for (uint32_t k = 0; k < template_frames; ++k) {
            const double a = 2.0 * kPi * hz[i] * (double)k / sample_rate, c = std::cos(a), s = std::sin(a);
            const double re = tmpl[2 * k], im = tmpl[2 * k + 1];
            o[2 * k] = (float)(re * c - im * s); o[2 * k + 1] = (float)(re * s + im * c);
        }
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_match_peaks(const float *row_peak, const uint32_t *row_at, const float *row_sum, size_t rows, const iqgpu_match_opts *o,
                                 double ratio, iqgpu_match_peak *out, size_t cap, size_t *n)
{
    const char *who = "iqgpu_match_peaks";
    if (n) *n = 0;
    const int rc = check_opts(o, who); if (rc) return rc;
    if (!n || (rows && (!row_peak || !row_at || !row_sum)) || (cap && !out)) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (!(ratio >= 0.0) || !std::isfinite(ratio)) return fail(IQGPU_EINVAL, "%s: ratio is not a finite number >= 0", who);
    const uint32_t nt = o->n_templates;
    const double B = (double)o->block_frames;
    size_t found = 0;
    for (size_t r = 0; r < rows; ++r) {
        for (uint32_t t = 0; t < nt; ++t) {
            const double pk = (double)row_peak[r * nt + t], rest = ((double)row_sum[r * nt + t] - pk) / (B - 1.0);
            if (!(pk > 0.0) || !(pk >= ratio * rest)) continue;
            if (found < cap) {
                iqgpu_match_peak &d = out[found];
                memset(&d, 0, sizeof(d));
                d.first_frame = (uint64_t)r * o->block_frames + row_at[r * nt + t];
                d.template_index = t; d.peak = row_peak[r * nt + t];
                d.ratio = rest > 0.0 ? pk / rest : HUGE_VAL;
            }
            ++found;
        }
    }
    *n = found;
    if (found > cap) return fail(IQGPU_ECAPACITY, "%s: room for %zu detections, the rows hold %zu", who, cap, found);
    return IQGPU_OK;
}
