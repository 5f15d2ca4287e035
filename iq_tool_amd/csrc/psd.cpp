// psd.cpp -- host side of the power-spectrum accumulator (include/iqgpu.h "power spectrum"; kernels psd.hip): the options,
// the window tables and the segment arithmetic (no device), and the iqgpu_psd handle -- stream position, the carry of trailing
// frames, the open page and the totals -- with push / push_device / read / reset.  Independent of any chain.
#include "chain.hpp"
#include "psd.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice

int log2n_of(uint32_t nfft) { return nfft == 1024 ? 10 : nfft == 2048 ? 11 : nfft == 4096 ? 12 : 0; }

int check_opts(const iqgpu_psd_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (!log2n_of(o->nfft)) return fail(IQGPU_EINVAL, "%s: nfft %u is not 1024, 2048 or 4096", who, o->nfft);
    if (o->hop != o->nfft && o->hop != o->nfft / 2 && o->hop != o->nfft / 4)
        return fail(IQGPU_EINVAL, "%s: hop %u is not nfft, nfft / 2 or nfft / 4 of nfft %u", who, o->hop, o->nfft);
    if (o->window < IQGPU_PSD_RECT || o->window > IQGPU_PSD_BLACKMAN_HARRIS) return fail(IQGPU_EINVAL, "%s: unknown window %d", who, o->window);
    if (!std::isfinite(o->gain)) return fail(IQGPU_EINVAL, "%s: gain is not finite", who);
    return IQGPU_OK;
}

// periodic (DFT-even) forms, evaluated in double, rounded once
float window_at(int window, uint32_t i, uint32_t n)
{
    const double di = (double)i, dn = (double)n;
    switch (window) {
    case IQGPU_PSD_HANN: return (float)(0.5 - 0.5 * std::cos(2.0 * kPi * di / dn));
    case IQGPU_PSD_HAMMING: return (float)(0.54 - 0.46 * std::cos(2.0 * kPi * di / dn));
    case IQGPU_PSD_BLACKMAN_HARRIS:
        return (float)(0.35875 - 0.48829 * std::cos(2.0 * kPi * di / dn) + 0.14128 * std::cos(4.0 * kPi * di / dn) - 0.01168 * std::cos(6.0 * kPi * di / dn));
    default: return 1.0f;
    }
}

void fill_window(const iqgpu_psd_opts &o, float *w, double *sum, double *sum_sq)
{
    double s = 0.0, q = 0.0;
    for (uint32_t i = 0; i < o.nfft; ++i) {
        w[i] = window_at(o.window, i, o.nfft);
        s += (double)w[i]; q += (double)w[i] * (double)w[i];
    }
    if (sum) *sum = s;
    if (sum_sq) *sum_sq = q;
}

uint64_t segments_of(const iqgpu_psd_opts &o, uint64_t frames) { return frames < o.nfft ? 0 : (frames - o.nfft) / o.hop + 1; }

} // namespace

// what sgram.cpp shares (psd.hpp): the same checks, table and grid, so the two accumulators cannot drift apart
namespace iqgpu {
int psd_check_opts(const iqgpu_psd_opts *o, const char *who) { return check_opts(o, who); }
void psd_fill_tables(const iqgpu_psd_opts &o, float *tab, double *sum, double *sum_sq)
{
    fill_window(o, tab, sum, sum_sq);
    for (uint32_t k = 0; k < o.nfft; ++k) {                           // exp(-2 pi i k / nfft): double, rounded once
        const double a = -2.0 * kPi * (double)k / (double)o.nfft;
        tab[o.nfft + 2 * k] = (float)std::cos(a); tab[o.nfft + 2 * k + 1] = (float)std::sin(a);
    }
}
uint64_t psd_segments_of(const iqgpu_psd_opts &o, uint64_t frames) { return segments_of(o, frames); }
int psd_log2n(uint32_t nfft) { return log2n_of(nfft); }
} // namespace iqgpu

struct iqgpu_psd {
    int device = 0, format = 0, log2n = 0;
    size_t bps = 0;
    iqgpu_psd_opts o{};
    double window_sum = 0.0, window_sum_sq = 0.0;
    uint64_t frames = 0, segments = 0;    // pushed since the last reset; whole segments of them (all accumulated)
    size_t carry_n = 0;                   // frames in carry[cur]: stream frames segments * hop .. frames - 1
    int cur = 0;
    int open_cur = 0;                     // which of the two open-page buffers holds the open page (the page kernel writes the other: psd.hip)
    bool poisoned = false;                // a push failed half way: reset() clears it
    hipStream_t own = nullptr, last = nullptr; bool has_last = false;     // last: the stream of the previous push
    hipEvent_t staged = nullptr;          // a host push: the slice has left the caller's memory
    DevBuf tables, carry[2], sums, pages, stage;
    size_t page_bins = 0;                 // of pages: [page_bins] doubles, then [page_bins] floats
    // tables: [nfft] window, [nfft] twiddles; sums: [nfft] total, 2 x [nfft] open (double), then [nfft] peak, 2 x [nfft] open peak (float)
    const float *window() const { return (const float *)tables.p; }
    const cf2 *twiddle() const { return (const cf2 *)((const float *)tables.p + o.nfft); }
    double *total_sum() const { return (double *)sums.p; }
    double *open_sum(int i) const { return (double *)sums.p + (size_t)(1 + i) * o.nfft; }
    float *total_pk() const { return (float *)((double *)sums.p + 3 * (size_t)o.nfft); }
    float *open_pk(int i) const { return total_pk() + (size_t)(1 + i) * o.nfft; }
    size_t sums_bytes() const { return (size_t)o.nfft * (3 * sizeof(double) + 3 * sizeof(float)); }
};

namespace {

void destroy(iqgpu_psd *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->has_last) (void)hipStreamSynchronize(p->last);
    if (p->own) { (void)hipStreamSynchronize(p->own); (void)hipStreamDestroy(p->own); }
    if (p->staged) (void)hipEventDestroy(p->staged);
    p->tables.release(); p->carry[0].release(); p->carry[1].release(); p->sums.release(); p->pages.release(); p->stage.release();
    delete p;
}

// everything queued by earlier pushes has run; the handle then holds on to no stream of the caller's
int settle(iqgpu_psd *p)
{
    if (p->has_last) HIP_TRY(hipStreamSynchronize(p->last));
    p->has_last = false; p->last = nullptr;
    return IQGPU_OK;
}

// n frames of device memory behind everything pushed so far, on s
int push_frames(iqgpu_psd *p, const void *d_raw, size_t n, hipStream_t s)
{
    if (p->has_last && p->last != s) HIP_TRY(hipStreamSynchronize(p->last));      // the previous push's work comes first
    p->has_last = true; p->last = s;
    const iqgpu_psd_opts &o = p->o;
    const int64_t G = kPsdPageSegments, cap = G * (kPsdPageBufBins / (int64_t)o.nfft);
    const uint64_t frames = p->frames + n, segs = segments_of(o, frames);
    const int64_t m = (int64_t)(segs - p->segments);
    // the page buffer: one slot for every page the longest launch of this push touches, the whole bound at most (sized before anything is
    // queued).  Growing it frees the old one while kernels of earlier pushes may still be queued on the caller's stream: that is safe because
    // hipFree waits for the device, and it makes the first long push of a handle wait once (iqgpu_psd_push's staging buffer: the same)
    const int64_t touched = m / G + 2;
    const size_t bins = (size_t)(touched * (int64_t)o.nfft < kPsdPageBufBins ? touched * (int64_t)o.nfft : kPsdPageBufBins);
    if (m > 0 && bins > p->page_bins) {
        const int rc = p->pages.ensure(bins * (sizeof(double) + sizeof(float))); if (rc) return rc;
        p->page_bins = bins;
    }
    p->poisoned = true;                                                           // (until everything below is queued)
    for (int64_t j = 0; j < m;) {
        const int64_t seg0 = (int64_t)p->segments + j;
        const int64_t cnt = m - j < cap - seg0 % G ? m - j : cap - seg0 % G;      // whole pages up to the page buffer's bound
        PsdPagesArgs a{};
        a.carry = p->carry[p->cur].p; a.raw = d_raw; a.split = (int64_t)p->carry_n; a.first = j * (int64_t)o.hop;
        a.fmt = p->format; a.log2n = p->log2n; a.hop = (int32_t)o.hop; a.gain = o.gain;
        a.seg0 = seg0; a.n_seg = cnt; a.window = p->window(); a.twiddle = p->twiddle();
        a.open_sum_in = p->open_sum(p->open_cur); a.open_pk_in = p->open_pk(p->open_cur);
        a.open_sum_out = p->open_sum(p->open_cur ^ 1); a.open_pk_out = p->open_pk(p->open_cur ^ 1);
        a.page_sum = (double *)p->pages.p; a.page_pk = (float *)((double *)p->pages.p + p->page_bins);
        HIP_TRY(launch_psd_pages(a, s));
        PsdFoldArgs f{};
        f.page_sum = a.page_sum; f.page_pk = a.page_pk; f.n_pages = (int32_t)((seg0 + cnt) / G - seg0 / G); f.nfft = (int32_t)o.nfft;
        f.total_sum = p->total_sum(); f.total_pk = p->total_pk();
        HIP_TRY(launch_psd_fold(f, s));
        if ((seg0 + cnt) % G != 0) p->open_cur ^= 1;                              // the launch left an open page, in the other buffer
        j += cnt;
    }
    // the trailing frames the next segment starts with, into the other buffer (the page kernels above read this one)
    const size_t carry_n = (size_t)(frames - segs * o.hop);
    PsdCarryArgs c{};
    c.carry = (const unsigned char *)p->carry[p->cur].p; c.raw = (const unsigned char *)d_raw;
    c.split_bytes = (int64_t)(p->carry_n * p->bps); c.first = (int64_t)((p->carry_n + n - carry_n) * p->bps);
    c.bytes = (int32_t)(carry_n * p->bps); c.dst = (unsigned char *)p->carry[p->cur ^ 1].p;
    HIP_TRY(launch_psd_carry(c, s));
    p->cur ^= 1; p->carry_n = carry_n; p->frames = frames; p->segments = segs;
    p->poisoned = false;
    return IQGPU_OK;
}

int begin_push(iqgpu_psd *p, const void *raw, const char *who)
{
    if (!p || !raw) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (p->poisoned) return fail(IQGPU_EHIP, "%s: an earlier push failed half way through: the accumulator is undefined until iqgpu_psd_reset()", who);
    HIP_TRY(hipSetDevice(p->device));
    return IQGPU_OK;
}

} // namespace

extern "C" void iqgpu_psd_opts_init(iqgpu_psd_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->nfft = 1024; o->hop = 512; o->window = IQGPU_PSD_HANN; o->gain = 1.0f;
}

extern "C" int iqgpu_psd_window(const iqgpu_psd_opts *o, float *w, size_t cap, double *sum, double *sum_sq)
{
    const int rc = check_opts(o, "iqgpu_psd_window"); if (rc) return rc;
    if (!w) return fail(IQGPU_EINVAL, "iqgpu_psd_window: NULL argument");
    if (cap < o->nfft) return fail(IQGPU_EINVAL, "iqgpu_psd_window: room for %zu values, the window has %u", cap, o->nfft);
    fill_window(*o, w, sum, sum_sq);
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_segments(const iqgpu_psd_opts *o, uint64_t frames, uint64_t *segments)
{
    const int rc = check_opts(o, "iqgpu_psd_segments"); if (rc) return rc;
    if (!segments) return fail(IQGPU_EINVAL, "iqgpu_psd_segments: NULL argument");
    *segments = segments_of(*o, frames);
    return IQGPU_OK;
}

extern "C" void iqgpu_psd_geometry(size_t *segments_per_page)
{
    if (segments_per_page) *segments_per_page = (size_t)kPsdPageSegments;
}

extern "C" int iqgpu_psd_create(int device, int format, const iqgpu_psd_opts *o, iqgpu_psd **out)
{
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "iqgpu_psd_create: NULL argument");
    int rc = check_opts(o, "iqgpu_psd_create"); if (rc) return rc;
    if (!bytes_per_frame(format)) return fail(IQGPU_EFORMAT, "iqgpu_psd_create: unhandled sample format %d", format);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(IQGPU_ENODEV, "iqgpu_psd_create: no HIP device available");
    if (device < 0 || device >= ndev) return fail(IQGPU_ENODEV, "iqgpu_psd_create: device %d out of range (%d devices)", device, ndev);
    iqgpu_psd *p = new (std::nothrow) iqgpu_psd;
    std::vector<float> tab;
    try { tab.resize(3 * (size_t)o->nfft); } catch (const std::bad_alloc &) { delete p; p = nullptr; }
    if (!p) return fail(IQGPU_ENOMEM, "iqgpu_psd_create: out of host memory");
    p->device = device; p->format = format; p->log2n = log2n_of(o->nfft); p->bps = bytes_per_frame(format); p->o = *o;
    psd_fill_tables(*o, tab.data(), &p->window_sum, &p->window_sum_sq);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->staged, hipEventDisableTiming);
    if (e != hipSuccess) { rc = fail(IQGPU_EHIP, "iqgpu_psd_create: %s", hipGetErrorString(e)); destroy(p); return rc; }
    rc = p->tables.ensure(tab.size() * sizeof(float));
    for (int i = 0; i < 2 && rc == IQGPU_OK; ++i) rc = p->carry[i].ensure((size_t)o->nfft * p->bps);
    if (rc == IQGPU_OK) rc = p->sums.ensure(p->sums_bytes());
    if (rc == IQGPU_OK) {
        e = hipMemcpyAsync(p->tables.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, p->own);
        if (e == hipSuccess) e = hipMemsetAsync(p->sums.p, 0, p->sums_bytes(), p->own);
        if (e == hipSuccess) e = hipStreamSynchronize(p->own);
        if (e != hipSuccess) rc = fail(IQGPU_EHIP, "iqgpu_psd_create: %s", hipGetErrorString(e));
    }
    if (rc != IQGPU_OK) { destroy(p); return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_psd_destroy(iqgpu_psd *p) { destroy(p); }

extern "C" int iqgpu_psd_reset(iqgpu_psd *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_psd_reset: NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    if (p->has_last) (void)hipStreamSynchronize(p->last);            // (a failed push may have left an error there: the fill below decides)
    HIP_TRY(hipMemsetAsync(p->sums.p, 0, p->sums_bytes(), p->own));
    HIP_TRY(hipStreamSynchronize(p->own));
    p->frames = p->segments = 0; p->carry_n = 0; p->cur = 0; p->open_cur = 0; p->has_last = false; p->last = nullptr; p->poisoned = false;
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_push_device(iqgpu_psd *p, const void *d_raw, size_t frames, void *hip_stream)
{
    if (p && frames == 0) return IQGPU_OK;
    const int rc = begin_push(p, d_raw, "iqgpu_psd_push_device"); if (rc) return rc;
    return push_frames(p, d_raw, frames, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_psd_push(iqgpu_psd *p, const void *raw, size_t frames)
{
    if (p && frames == 0) return IQGPU_OK;
    int rc = begin_push(p, raw, "iqgpu_psd_push"); if (rc) return rc;
    rc = p->stage.ensure((frames < kPushSliceFrames ? frames : kPushSliceFrames) * p->bps); if (rc) return rc;
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < kPushSliceFrames ? frames - at : kPushSliceFrames;
        // (the one staging buffer: the copy is ordered behind the kernels of the slice in front on the handle's stream)
        HIP_TRY(hipMemcpyAsync(p->stage.p, (const char *)raw + at * p->bps, n * p->bps, hipMemcpyHostToDevice, p->own));
        HIP_TRY(hipEventRecord(p->staged, p->own));
        rc = push_frames(p, p->stage.p, n, p->own); if (rc) return rc;
        HIP_TRY(hipEventSynchronize(p->staged));                     // the caller's memory is free when the call returns
        at += n;
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_read(iqgpu_psd *p, double *sum_power, float *peak_power, iqgpu_psd_info *info)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_psd_read: NULL argument");
    if (p->poisoned) return fail(IQGPU_EHIP, "iqgpu_psd_read: an earlier push failed half way through: the accumulator is undefined until iqgpu_psd_reset()");
    HIP_TRY(hipSetDevice(p->device));
    int rc = settle(p); if (rc) return rc;
    const size_t n = p->o.nfft;
    if (sum_power || peak_power) {
        std::vector<double> s; std::vector<float> k;
        try { s.resize(2 * n); k.resize(2 * n); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "iqgpu_psd_read: out of host memory"); }
        HIP_TRY(hipMemcpy(s.data(), p->total_sum(), n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(s.data() + n, p->open_sum(p->open_cur), n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(k.data(), p->total_pk(), n * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(k.data() + n, p->open_pk(p->open_cur), n * sizeof(float), hipMemcpyDeviceToHost));
        const bool open = p->segments % (uint64_t)kPsdPageSegments != 0;      // else the open arrays hold a page already folded
        for (size_t i = 0; i < n; ++i) {
            if (sum_power) sum_power[i] = open ? s[i] + s[n + i] : s[i];
            if (peak_power) peak_power[i] = open ? fmaxf(k[i], k[n + i]) : k[i];
        }
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->frames = p->frames; info->segments = p->segments; info->nfft = p->o.nfft; info->hop = p->o.hop;
        info->window_sum = p->window_sum; info->window_sum_sq = p->window_sum_sq;
    }
    return IQGPU_OK;
}
