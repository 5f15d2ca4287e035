// iq_calib.cpp -- host side of the I/Q calibration on the device (include/iqgpu.h "I/Q calibration"): iqgpu_iq_metric_batch[_device],
// iqgpu_chain_calibrate_iq[_device] and the block gather behind them.  The search is iq_calib_search (iq_optimizer.cpp, the one the
// host calibration runs); here is its second evaluator, k_iq_metric, and what feeds it.  A chain call works in buffers of its own
// (iqgpu_chain::iq_cal_*) on the chain's stream and reads nothing the stream carries but the description's constants.
#include "chain.hpp"
#include "iq_calib.hpp"

namespace {

constexpr size_t kMaxBlocks = (size_t)1 << 20;       // of one call: 2^30 input frames' worth

// window: the optimiser's float expression (iq_optimizer.cpp create, iq_correct.c:122-124); twiddles: double, rounded once
struct IqTables { float window[kIqN]; cf2 tw[kIqN]; };
const IqTables &iq_tables()
{
    static const IqTables t = [] {
        IqTables x;
        for (int i = 0; i < kIqN; ++i)
            x.window[i] = 0.54f - 0.46f * cosf(2.0f * (float)3.14159265358979323846 * (float)i / (float)(kIqN - 1));
        for (int k = 0; k < kIqN; ++k) {
            const double a = -2.0 * 3.14159265358979323846 * (double)k / (double)kIqN;
            x.tw[k] = cf2{(float)std::cos(a), (float)std::sin(a)};
        }
        return x;
    }();
    return t;
}

int ensure_tables(DevBuf &tab, hipStream_t s)
{
    if (tab.p) return IQGPU_OK;
    DevBuf nb;                                                        // (allocated = uploaded: tab takes it once the copy is queued)
    const int rc = nb.ensure(sizeof(IqTables)); if (rc) return rc;
    const hipError_t e = hipMemcpyAsync(nb.p, &iq_tables(), sizeof(IqTables), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return fail(IQGPU_EHIP, "uploading the calibration tables failed: %s", hipGetErrorString(e));
    tab = std::move(nb);
    return IQGPU_OK;
}

// the device evaluator: k_iq_metric over cf32 blocks in device memory, at most kIqCandsPerLaunch candidates a launch
struct DevEval {
    hipStream_t s; const cf2 *d_blocks; int64_t stride; size_t n_blocks;
    const IqTables *d_tab; DevBuf *work;
};

int dev_eval(void *user, const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db)
{
    const DevEval &e = *(const DevEval *)user;
    const size_t cand_bytes = (n_cand * sizeof(iqgpu_iq_cand) + 255) & ~(size_t)255;
    const size_t metric_bytes = (e.n_blocks * n_cand * sizeof(float) + 255) & ~(size_t)255;
    int rc = e.work->ensure(cand_bytes + metric_bytes + e.n_blocks * 2 * sizeof(float)); if (rc) return rc;
    iqgpu_iq_cand *d_cand = (iqgpu_iq_cand *)e.work->p;
    float *d_metric = (float *)((char *)e.work->p + cand_bytes);
    float *d_power = (float *)((char *)e.work->p + cand_bytes + metric_bytes);
    HIP_TRY(hipMemcpyAsync(d_cand, cands, n_cand * sizeof(iqgpu_iq_cand), hipMemcpyHostToDevice, e.s));
    for (size_t c0 = 0; c0 < n_cand; c0 += (size_t)kIqCandsPerLaunch) {
        IqMetricArgs a{};
        a.blocks = e.d_blocks; a.stride = e.stride; a.n_blocks = (int32_t)e.n_blocks;
        a.n_cand = (int32_t)(n_cand - c0 < (size_t)kIqCandsPerLaunch ? n_cand - c0 : (size_t)kIqCandsPerLaunch);
        a.cands = d_cand + c0; a.window = e.d_tab->window; a.twiddle = e.d_tab->tw;
        a.metric = d_metric + c0; a.metric_pitch = (int64_t)n_cand;
        a.power = (power_range_db && c0 == 0) ? d_power : nullptr;
        HIP_TRY(launch_iq_metric(a, e.s));
    }
    std::vector<float> power;
    if (power_range_db) {
        try { power.resize(e.n_blocks * 2); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "out of host memory"); }
        HIP_TRY(hipMemcpyAsync(power.data(), d_power, e.n_blocks * 2 * sizeof(float), hipMemcpyDeviceToHost, e.s));
    }
    HIP_TRY(hipMemcpyAsync(metric, d_metric, e.n_blocks * n_cand * sizeof(float), hipMemcpyDeviceToHost, e.s));
    HIP_TRY(hipStreamSynchronize(e.s));
    if (power_range_db) for (size_t b = 0; b < e.n_blocks; ++b) power_range_db[b] = power[2 * b + 1];
    return IQGPU_OK;
}

int metric_batch_impl(int device, const float *blocks, size_t n_blocks, size_t stride, const iqgpu_iq_cand *cands, size_t n_cand,
                      float *metric, float *power_range_db, bool on_device, hipStream_t s)
{
    const char *who = on_device ? "iqgpu_iq_metric_batch_device" : "iqgpu_iq_metric_batch";
    if (!blocks || !cands || !metric) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (n_blocks == 0 || n_cand == 0) return fail(IQGPU_EINVAL, "%s: no blocks or no candidates", who);
    if (stride < (size_t)kIqN) return fail(IQGPU_EINVAL, "%s: stride_frames %zu is below %d", who, stride, kIqN);
    if (n_blocks > kMaxBlocks || n_cand > ((size_t)1 << 31) / n_blocks) return fail(IQGPU_EINVAL, "%s: %zu blocks x %zu candidates is too many for one call", who, n_blocks, n_cand);
    HIP_TRY(hipSetDevice(device));
    DevBuf tab, in, work;
    int rc = ensure_tables(tab, s);
    const cf2 *d_blocks = (const cf2 *)blocks;
    int64_t d_stride = (int64_t)stride;
    if (rc == IQGPU_OK && !on_device) {                               // the blocks, not the gaps between them
        rc = in.ensure(n_blocks * kIqN * sizeof(cf2));
        hipError_t e = hipSuccess;
        for (size_t b = 0; rc == IQGPU_OK && b < n_blocks && e == hipSuccess; ++b)
            e = hipMemcpyAsync((cf2 *)in.p + b * kIqN, blocks + 2 * b * stride, kIqN * sizeof(cf2), hipMemcpyHostToDevice, s);
        if (rc == IQGPU_OK && e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: copying the blocks failed: %s", who, hipGetErrorString(e));
        d_blocks = (const cf2 *)in.p; d_stride = kIqN;
    }
    if (rc == IQGPU_OK) {
        DevEval ev{s, d_blocks, d_stride, n_blocks, (const IqTables *)tab.p, &work};
        rc = dev_eval(&ev, cands, n_cand, metric, power_range_db);
    }
    (void)hipStreamSynchronize(s);                                    // (an error path: nothing in flight reads what tab, in and work free next)
    return rc;
}

// n blocks, block b at frame b * stride (include/iqgpu.h)
void select_blocks(size_t frames_in, uint32_t max_blocks, size_t *n, size_t *stride)
{
    size_t k = frames_in / (size_t)kIqN;
    if (k > (size_t)max_blocks) k = max_blocks;
    if (k > kMaxBlocks) k = kMaxBlocks;
    *n = k;
    *stride = frames_in / k > (size_t)kIqN ? frames_in / k : (size_t)kIqN;
}

// the selected blocks of raw input, as cf32 in c->iq_cal_blocks (queued on the chain's stream)
int gather_blocks(iqgpu_chain *c, const void *in, size_t n, size_t stride, bool on_device)
{
    int rc = c->iq_cal_blocks.ensure(n * kIqN * sizeof(cf2)); if (rc) return rc;
    const size_t ibps = bytes_per_frame(c->desc.in_format);
    const void *d_in = in;
    int64_t d_stride = (int64_t)stride;
    if (!on_device) {                                                 // the host form stages the blocks it needs, not the whole input
        rc = c->iq_cal_in.ensure(n * kIqN * ibps); if (rc) return rc;
        for (size_t b = 0; b < n; ++b)
            HIP_TRY(hipMemcpyAsync((char *)c->iq_cal_in.p + b * kIqN * ibps, (const char *)in + b * stride * ibps, kIqN * ibps,
                                   hipMemcpyHostToDevice, c->stream));
        d_in = c->iq_cal_in.p; d_stride = kIqN;
    }
    IqBlocksArgs a{};
    a.raw = d_in; a.in_fmt = c->desc.in_format; a.gain = c->desc.gain;
    a.dc_enable = c->dc ? 1 : 0; a.dc_c = c->dc_c;
    a.stride = d_stride; a.n_blocks = (int32_t)n; a.out = (cf2 *)c->iq_cal_blocks.p;
    HIP_TRY(launch_iq_blocks(a, c->stream));
    return IQGPU_OK;
}

// what both chain calls start with: arguments, the batches in flight, the selection, the gather
int begin_chain_call(iqgpu_chain *c, const void *in, size_t frames_in, uint32_t max_blocks, bool on_device, const char *who, size_t *n)
{
    if (!c || !in) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (max_blocks == 0) return fail(IQGPU_EINVAL, "%s: max_blocks must be positive", who);
    if (frames_in < (size_t)kIqN) return fail(IQGPU_EINVAL, "%s: %zu frames are less than one block of %d", who, frames_in, kIqN);
    if (c->poisoned) return fail(IQGPU_EHIP, "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    int rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;         // batches submitted earlier come first (same stream)
    size_t stride = 0;
    select_blocks(frames_in, max_blocks, n, &stride);
    return gather_blocks(c, in, *n, stride, on_device);
}

int calibrate_impl(iqgpu_chain *c, const void *in, size_t frames_in, const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep, bool on_device)
{
    const char *who = on_device ? "iqgpu_chain_calibrate_iq_device" : "iqgpu_chain_calibrate_iq";
    if (rep) memset(rep, 0, sizeof(*rep));
    if (!rep) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    const char *why = nullptr;
    if (iq_calib_check_opts(opts, &why) != IQGPU_OK) return fail(IQGPU_EINVAL, "%s: %s", who, why);
    size_t n = 0;
    int rc = begin_chain_call(c, in, frames_in, opts->max_blocks, on_device, who, &n);
    if (rc == IQGPU_OK) rc = ensure_tables(c->iq_cal_tab, c->stream);
    if (rc == IQGPU_OK) {
        DevEval ev{c->stream, (const cf2 *)c->iq_cal_blocks.p, kIqN, n, (const IqTables *)c->iq_cal_tab.p, &c->iq_cal_work};
        rc = iq_calib_search(*opts, n, dev_eval, &ev, rep);
        if (rc == IQGPU_ENOMEM) (void)fail(rc, "%s: out of memory", who);
    }
    if (c && !c->poisoned && c->stream) (void)hipStreamSynchronize(c->stream);     // idle on every path (dev_eval has waited on the good one)
    return rc;
}

int blocks_impl(iqgpu_chain *c, const void *in, size_t frames_in, uint32_t max_blocks, float *blocks, size_t cap, size_t *n_blocks, bool on_device)
{
    const char *who = on_device ? "iqgpu_chain_calibrate_iq_blocks_device" : "iqgpu_chain_calibrate_iq_blocks";
    if (n_blocks) *n_blocks = 0;
    if (!blocks || !n_blocks) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    size_t n = 0;
    int rc = begin_chain_call(c, in, frames_in, max_blocks, on_device, who, &n);
    if (rc == IQGPU_OK && n > cap) rc = fail(IQGPU_ECAPACITY, "%s: %zu blocks, room for %zu", who, n, cap);
    hipError_t e = hipSuccess;
    if (rc == IQGPU_OK) e = hipMemcpyAsync(blocks, c->iq_cal_blocks.p, n * kIqN * sizeof(cf2), hipMemcpyDeviceToHost, c->stream);
    if (c && !c->poisoned && c->stream) { const hipError_t e2 = hipStreamSynchronize(c->stream); if (e == hipSuccess) e = e2; }
    if (rc == IQGPU_OK && e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    if (rc == IQGPU_OK) *n_blocks = n;
    return rc;
}

} // namespace

extern "C" void iqgpu_iq_metric_geometry(size_t *cands_per_launch, size_t *cand_tile)
{
    if (cands_per_launch) *cands_per_launch = (size_t)kIqCandsPerLaunch;
    if (cand_tile) *cand_tile = (size_t)kIqCandTile;
}

extern "C" int iqgpu_iq_metric_batch(int device, const float *blocks_re_im, size_t n_blocks, size_t stride_frames,
                                     const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db)
{
    return metric_batch_impl(device, blocks_re_im, n_blocks, stride_frames, cands, n_cand, metric, power_range_db, false, nullptr);
}
extern "C" int iqgpu_iq_metric_batch_device(int device, const float *d_blocks_re_im, size_t n_blocks, size_t stride_frames,
                                            const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db, void *hip_stream)
{
    return metric_batch_impl(device, d_blocks_re_im, n_blocks, stride_frames, cands, n_cand, metric, power_range_db, true, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_chain_calibrate_iq(iqgpu_chain *c, const void *raw_in, size_t frames_in,
                                        const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep)
{
    return calibrate_impl(c, raw_in, frames_in, opts, rep, false);
}
extern "C" int iqgpu_chain_calibrate_iq_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                                               const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep)
{
    return calibrate_impl(c, d_raw_in, frames_in, opts, rep, true);
}
extern "C" int iqgpu_chain_calibrate_iq_blocks(iqgpu_chain *c, const void *raw_in, size_t frames_in, uint32_t max_blocks,
                                               float *blocks_re_im, size_t cap_blocks, size_t *n_blocks)
{
    return blocks_impl(c, raw_in, frames_in, max_blocks, blocks_re_im, cap_blocks, n_blocks, false);
}
extern "C" int iqgpu_chain_calibrate_iq_blocks_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, uint32_t max_blocks,
                                                      float *blocks_re_im, size_t cap_blocks, size_t *n_blocks)
{
    return blocks_impl(c, d_raw_in, frames_in, max_blocks, blocks_re_im, cap_blocks, n_blocks, true);
}
