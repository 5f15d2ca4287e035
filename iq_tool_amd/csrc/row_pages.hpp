// row_pages.hpp -- the host core of the accumulators that emit rows per block of B frames over iqgpu_env's page geometry (env.hpp):
// iqgpu_env (env.cpp) and iqgpu_lag (lag.cpp).  The handle core (accum_core.hpp), B, the open row in two records flipped behind
// every launch, the slab of a launch, the staging pair of a host push, and, each defined once: the block_frames check, the rows of
// a push, the cut of a push into launches of whole pages below 2^28 frames with the fold's arithmetic, and what of the open row is
// where.  What a record holds and what a launch's arguments are is the accumulator's.
#pragma once
#include "accum_core.hpp"
#include "env.hpp"

namespace iqgpu {

// one launch of a push, as the cut hands it to the accumulator: the frames, the grid, and the fold's arithmetic
struct RowLaunch {
    const char *raw;              // device memory, frame `first` of the stream
    uint64_t first, cnt, end;
    int groups, pages_per_group;
    bool cf32;
    int32_t log2_cells_per_row;
    int64_t c0, n_closed, n_touched, rows_before;
    uint64_t done;                // rows the launch finishes
};

// what of the open row is where: its closed cells in the record's total (has_tot), its open page in the record's columns (has_page),
// of which the row's terms are columns [at, at + cnt)
struct OpenRow { uint64_t open_frames; bool has_tot, has_page; size_t at, cnt; };

struct IQGPU_LOCAL RowPages : AccumCore {
    int log2_b = 0;
    int open_cur = 0;                     // which open record holds the open row (a launch writes the other)
    size_t open_bytes = 0, cell_bytes = 0;
    // state: 2 x the open record, then the non-finite total (uint64); slab: [kEnvMaxGroups] uint32, then [kEnvMaxCells] cells (B > 65536)
    DevBuf state, slab, stage, rows_out;

    // log2 of a valid block_frames, -1 otherwise
    static int log2_block(uint32_t b)
    {
        if (b == 0 || (b & (b - 1)) != 0) return -1;
        int l = 0;
        while (((uint32_t)1 << l) != b) ++l;
        return l >= kEnvLog2BlockMin && l <= kEnvLog2BlockMax ? l : -1;
    }
    static int check_block(uint32_t b, const char *who)
    {
        if (log2_block(b) < 0)
            return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^%d .. 2^%d", who, b, kEnvLog2BlockMin, kEnvLog2BlockMax);
        return IQGPU_OK;
    }
    uint64_t B() const { return (uint64_t)1 << log2_b; }
    size_t rows_of(size_t n) const { return (size_t)(((frames + n) >> log2_b) - (frames >> log2_b)); }
    void *open_rec(int i) const { return (char *)state.p + (size_t)i * open_bytes; }
    uint64_t *nonfinite_total() const { return (uint64_t *)((char *)state.p + 2 * open_bytes); }
    size_t state_bytes() const { return 2 * open_bytes + sizeof(uint64_t); }
    uint32_t *slab_nonfinite() const { return (uint32_t *)slab.p; }
    void *slab_cells() const { return log2_b > kEnvLog2CellFrames ? (void *)((uint32_t *)slab.p + kEnvMaxGroups) : nullptr; }
    size_t slab_bytes() const { return (size_t)kEnvMaxGroups * sizeof(uint32_t) + (log2_b > kEnvLog2CellFrames ? (size_t)kEnvMaxCells * cell_bytes : 0); }

    // AccumCore::open, then the state and the slab for records of open_bytes and cells of cell_bytes (the caller's own buffers and
    // zero_state() follow)
    static int open(RowPages *rp, int device, int format, uint32_t block_frames, size_t open_bytes, size_t cell_bytes, const char *who)
    {
        int rc = AccumCore::open(rp, device, format, who); if (rc) return rc;
        rp->log2_b = log2_block(block_frames); rp->open_bytes = open_bytes; rp->cell_bytes = cell_bytes;
        rc = rp->state.ensure(rp->state_bytes()); if (rc) return rc;
        return rp->slab.ensure(rp->slab_bytes());
    }
    int zero_state()
    {
        HIP_TRY(hipMemsetAsync(state.p, 0, state_bytes(), own));
        HIP_TRY(hipStreamSynchronize(own));
        return IQGPU_OK;
    }
    static int reset(RowPages *rp, const char *who)
    {
        if (!rp) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
        int rc = rp->begin_reset(); if (rc) return rc;
        rc = rp->zero_state(); if (rc) return rc;
        rp->rewind(); rp->open_cur = 0;
        return IQGPU_OK;
    }
    // the checks of both pushes, in front of anything queued; *need = the rows the push finishes
    static int begin_push(RowPages *rp, const void *raw, size_t frames, bool planes, size_t cap_rows, size_t *rows, size_t *need, const char *who,
                          const char *reset_name, const char *max_rows_name)
    {
        if (rows) *rows = 0;
        const int rc = guard(rp, raw || !frames, who, reset_name, false); if (rc) return rc;
        *need = rp->rows_of(frames);
        if (planes && *need > cap_rows)
            return fail(IQGPU_ECAPACITY, "%s: room for %zu rows, the push finishes %zu (%s)", who, cap_rows, *need, max_rows_name);
        if (frames) HIP_TRY(hipSetDevice(rp->device));
        return IQGPU_OK;
    }
    // n frames of device memory behind everything pushed so far, on s: cut into launches of whole pages up to the launch's bound,
    // each handed to launch(const RowLaunch &), which reads open_cur as the launch finds it; the flip and the position behind it
    template <class Launch> int push(const void *d_raw, size_t n, hipStream_t s, Launch launch)
    {
        int rc = note_stream(s); if (rc) return rc;
        const int lb = log2_b, lp = env_log2_page(lb);
        const uint64_t P = (uint64_t)1 << lp;
        poisoned = true;                                                          // (until the last launch of the push is queued)
        for (size_t at = 0; at < n;) {
            RowLaunch u{};
            u.first = frames;
            const uint64_t room = ((uint64_t)1 << kEnvLog2LaunchFrames) - u.first % P;    // whole pages up to the launch's bound
            u.cnt = n - at < room ? n - at : room; u.end = u.first + u.cnt;
            u.raw = (const char *)d_raw + at * bps;
            env_grid((int64_t)u.first, (int64_t)u.cnt, lb, &u.groups, &u.pages_per_group);
            u.cf32 = format == IQGPU_FMT_CF32;
            u.log2_cells_per_row = lb > kEnvLog2CellFrames ? lb - kEnvLog2CellFrames : 0;
            u.c0 = (int64_t)(u.first >> lp); u.n_closed = (int64_t)((u.end >> lp) - (u.first >> lp));
            u.n_touched = (int64_t)(((u.end - 1) >> lp) - (u.first >> lp) + 1);
            u.rows_before = (int64_t)(u.first >> lb);
            u.done = (u.end >> lb) - (u.first >> lb);
            rc = launch(u); if (rc) return rc;
            open_cur ^= 1;                                                        // the open row, if the launch left one, is in the other record
            frames = u.end;
            at += (size_t)u.cnt;
        }
        poisoned = false;
        return IQGPU_OK;
    }
    // the fold's arguments that every accumulator's fold block has (Fold: EnvFoldArgs, LagFoldArgs), but for cells, records and planes
    template <class Fold> void fill_fold(const RowLaunch &u, Fold *f) const
    {
        f->nonfinite = slab_nonfinite(); f->n_groups = u.cf32 ? u.groups : 0; f->nonfinite_total = nonfinite_total();
        f->log2_cells_per_row = u.log2_cells_per_row;
        f->c0 = u.c0; f->n_closed = u.n_closed; f->n_touched = u.n_touched; f->rows_before = u.rows_before;
    }

    // read_open: what the arithmetic says is there -- what it says is empty is not looked at.  B < 1024: the open row's terms are
    // columns [at, at + open_frames) of the step
    OpenRow open_row() const
    {
        OpenRow r;
        const uint64_t P = (uint64_t)1 << env_log2_page(log2_b);
        r.open_frames = frames % B();
        r.has_tot = r.open_frames >= (uint64_t)kStatsPageFrames; r.has_page = frames % P != 0 && r.open_frames != 0;
        r.at = B() < (uint64_t)kStatsColumns ? (size_t)((frames - r.open_frames) % kStatsColumns) : 0;
        r.cnt = B() < (uint64_t)kStatsColumns ? (size_t)r.open_frames : (size_t)kStatsColumns;
        return r;
    }
    // the open record into host memory: whole with an open page, else from its total (at tot_offset, the record's last part) on
    int fetch_open(const OpenRow &r, void *rec, size_t tot_offset) const
    {
        const size_t from = r.has_page ? 0 : tot_offset;
        HIP_TRY(hipMemcpy((char *)rec + from, (const char *)open_rec(open_cur) + from, open_bytes - from, hipMemcpyDeviceToHost));
        return IQGPU_OK;
    }
    // the tree over the open row's terms of one component: the tree over B terms is the tree over 1024 columns whose others are +0.0
    static double open_tree(const OpenRow &r, const double *col)
    {
        double t[kStatsColumns] = {0.0};
        for (size_t i = 0; i < r.cnt; ++i) t[i] = col[r.at + i];
        return stats_tree(t);
    }
};

} // namespace iqgpu
