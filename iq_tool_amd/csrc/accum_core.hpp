// accum_core.hpp -- what the five stream accumulators' handles have in common on the host (iqgpu_psd and iqgpu_sgram through
// PsdStream, psd.hpp; iqgpu_stats, stats.cpp; iqgpu_env and iqgpu_lag through RowPages, row_pages.hpp): the identity, the position in
// the stream, the stream of its own and the one of the previous push, the poisoned flag of a push that failed half way -- one
// definition of that protocol -- and the loop of a host push whose rows come back slice by slice (env, lag, sgram).
#pragma once
#include "chain.hpp"

namespace iqgpu {

struct IQGPU_LOCAL AccumCore {
    int device = 0, format = 0;
    size_t bps = 0;
    uint64_t frames = 0;                  // pushed since the last reset
    bool poisoned = false;                // a push failed half way: rewind() clears it
    Stream own; hipStream_t last = nullptr; bool has_last = false;        // last: the stream of the previous push (not owned)

    // The checks of a create in their order -- format, device count and range, host memory (c NULL: no handle could be allocated) --
    // then the device and the stream.  `who` leads the error texts.
    static int open(AccumCore *c, int device, int format, const char *who)
    {
        if (!bytes_per_frame(format)) return fail(IQGPU_EFORMAT, "%s: unhandled sample format %d", who, format);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(IQGPU_ENODEV, "%s: no HIP device available", who);
        if (device < 0 || device >= ndev) return fail(IQGPU_ENODEV, "%s: device %d out of range (%d devices)", who, device, ndev);
        if (!c) return fail(IQGPU_ENOMEM, "%s: out of host memory", who);
        c->device = device; c->format = format; c->bps = bytes_per_frame(format);
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = c->own.create();
        return e == hipSuccess ? IQGPU_OK : fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    // waits for `last` and `own`: the holder's destructor calls it in front of the members' frees
    void close()
    {
        if (!own) return;                 // (open() got no further than its checks: nothing is held)
        (void)hipSetDevice(device);
        if (has_last) (void)hipStreamSynchronize(last);
        (void)hipStreamSynchronize(own);
    }
    // NULL (c, or !args_ok) and poisoned, in the handles' texts (`reset` names the call that clears a poisoned handle), then hipSetDevice
    static int guard(const AccumCore *c, bool args_ok, const char *who, const char *reset, bool set_device = true)
    {
        if (!c || !args_ok) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
        if (c->poisoned) return fail(IQGPU_EHIP, "%s: an earlier push failed half way through: the accumulator is undefined until %s()", who, reset);
        if (set_device) HIP_TRY(hipSetDevice(c->device));
        return IQGPU_OK;
    }
    // everything queued by earlier pushes has run; the handle then holds on to no stream of the caller's
    int settle()
    {
        if (has_last) HIP_TRY(hipStreamSynchronize(last));
        has_last = false; last = nullptr;
        return IQGPU_OK;
    }
    // a reset: `last` waited for (a failed push may have left an error there: ignored), the caller zero-fills its state on `own`, then
    int begin_reset() { HIP_TRY(hipSetDevice(device)); if (has_last) (void)hipStreamSynchronize(last); return IQGPU_OK; }
    void rewind() { frames = 0; has_last = false; last = nullptr; poisoned = false; }     // ... as created
    // a push on s: the previous push's work comes first if its stream is another; s remembered
    int note_stream(hipStream_t s)
    {
        if (has_last && last != s) HIP_TRY(hipStreamSynchronize(last));
        has_last = true; last = s;
        return IQGPU_OK;
    }
};

// one plane of rows of a host push: the caller's memory (NULL: not asked for), the device rows of a slice, the bytes of a row
struct HostPlane { char *host; const void *dev; size_t row_bytes; };

// The host push of an accumulator whose rows come back: `frames` frames at raw in slices of at most slice_frames, each staged in
// `stage` (sized by the caller), pushed on the handle's stream by push(d_raw, n) and synchronised behind the copy of the rows it
// finishes (rows_of(n), slice_rows at most) into the planes: the one staging pair.  `who` and `verb` make the refusal's text.
template <int n_planes, class RowsOf, class Push>
int push_host_slices(AccumCore &c, DevBuf &stage, const void *raw, size_t frames, size_t slice_frames, size_t slice_rows,
                     HostPlane (&planes)[n_planes], const char *who, const char *verb, RowsOf rows_of, Push push)
{
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < slice_frames ? frames - at : slice_frames;
        const size_t done = rows_of(n);
        if (done > slice_rows) return fail(IQGPU_EHIP, "%s: a slice %s %zu rows, the buffer holds %zu", who, verb, done, slice_rows);
        HIP_TRY(hipMemcpyAsync(stage.p, (const char *)raw + at * c.bps, n * c.bps, hipMemcpyHostToDevice, c.own));
        const int rc = push(stage.p, n); if (rc) return rc;
        c.poisoned = true;                                               // (until the slice's rows are in the caller's memory)
        for (int i = 0; i < n_planes; ++i)
            if (planes[i].host && done) HIP_TRY(hipMemcpyAsync(planes[i].host, planes[i].dev, done * planes[i].row_bytes, hipMemcpyDeviceToHost, c.own));
        HIP_TRY(hipStreamSynchronize(c.own));
        c.poisoned = false;
        for (int i = 0; i < n_planes; ++i)
            if (planes[i].host) planes[i].host += done * planes[i].row_bytes;
        at += n;
    }
    return IQGPU_OK;
}

} // namespace iqgpu
