/*
 * iqgpu_run -- minimal raw-file harness around libiqgpu: reader -> GPU chain -> writer.
 *
 * It plays the role that iq_tool's raw-file reader (src/input_rawfile.c:168-252), stage threads and
 * raw-file writer (src/output_raw_file.c:146-184) play around the sample path, with the reference's
 * option names where they exist, so that BASELINE.json's configs can be run from a shell:
 *
 *   iqgpu_run -i in.cs16 --raw-file-input-rate 2.4e6 --raw-file-input-sample-format cs16 \
 *             -o out.cs16 --output-rate 744187.5 --output-sample-format cs16 --freq-shift 200e3
 *
 * Copies are double-buffered: pinned host buffers, hipMemcpyAsync on separate streams, events
 * between them (all through the C ABI, no HIP header here), so H2D of chunk i+1 and D2H of chunk
 * i-1 overlap the kernels of chunk i.  Nothing is flushed at end of stream (as in the reference).
 *
 * --shards N splits the input file into N equal frame ranges, one worker thread (and one GPU,
 * round-robin over --devices) per range, each with fresh state, and stitches the outputs in shard
 * order with pwrite at offsets known up front (the output count of a shard is a closed form):
 * exactly what N iq_tool runs + cat would produce (BASELINE configs[4]).  No collective.  Every shard thread binds itself to
 * the NUMA node of its GPU before its first GPU call and before it allocates its pinned buffers (iqgpu_bind_thread_to_device),
 * and fails when the frames its chain produced differ from the count its output offset was planned with.
 *
 * --shards N --seamless cuts ONE stream instead: shard starts are s * (frames / N) rounded down to a multiple of 4096 frames (every
 * 2^S decimation group the ratio range allows and 16 bytes of every input format divide it, so each shard starts on a group and on
 * an aligned word), every shard thread reads the iqgpu_design_preroll_frames frames in front of its start, puts its chain there with
 * iqgpu_chain_seek and runs its usual chunk loop; output offsets come from iqgpu_design_out_frames_range.  The stitched file is the
 * file --shards 1 writes (iqgpu.h: byte for byte without --dc-block, to 1e-6 of full scale with it; refused with an AGC option).
 *
 * --shards N --seamless-agc is --seamless for chains with the digital output AGC (every shipped preset), in the two passes of
 * iqgpu.h's v8 block.  Shard starts are s * (frames / N) rounded down to a multiple of lcm(4096, AGC chunk, --chunk-frames): the
 * digital AGC works on the chunks of each call, so every call of every shard has to lie on the single stream's call and chunk grid.
 * Pass 1: shards 0 .. N-2 put their chain at their start (iqgpu_chain_seek_agc, no entry state) and measure their range batch by
 * batch (iqgpu_chain_measure; the last shard's range is in front of nobody).  One walk over the tables in order
 * (iqgpu_chain_agc_advance) then gives the AGC state at the start of shards 1 .. N-1.  Pass 2: every shard seeks again, now with
 * its entry state, and runs the usual chunk loop.  Preroll and output placement come from the description with the AGC off.
 *
 * --shards N --seamless-dc is the EXACT --seamless for chains with the DC blocker (--dc-block, no AGC option), in the three passes of
 * iqgpu.h's DC block.  Shard starts are s * (frames / N) rounded down to a multiple of lcm(4096, --chunk-frames): every call of every
 * shard is a call of the single stream.  Pass 1: shards 0 .. N-2 measure the map of every call of their range
 * (iqgpu_chain_dc_measure: one read of the input, no front kernel, no output).  One walk over all rows (iqgpu_chain_dc_advance) then
 * gives the blocker's state in front of every call.  Pass 2: every shard puts its chain at its start with iqgpu_chain_seek_dc -- the
 * preroll is the filters' memory rounded up to whole chunks, with NO warm-up of the blocker, entered with the walked state -- and runs
 * the usual chunk loop.  The stitched file is the file --shards 1 writes, byte for byte.
 *
 * --shards N --seamless-rms is --seamless for chains with the dx / local output AGC (--output-agc, --agc-profile dx|local), whose
 * loop state the library rebuilds from a bounded window (iqgpu.h): cuts at multiples of 4096 frames, every shard thread reads the
 * iqgpu_design_preroll_frames_rms frames in front of its start, seeks with iqgpu_chain_seek_rms, processes its range and records its
 * AGC state right after the seek and behind the range, and a checkpoint behind the range.  After the join the seams are checked in
 * order: the state a shard started from against the state the shard in front ended in (gain, peak_memory, samples_seen, bit for
 * bit).  A range behind a seam that does not certify -- a cut in or behind digital silence -- is processed again from the checkpoint
 * of the range in front, and the next seam is checked against its new end state.  The file is the one --shards 1 writes; the report
 * says how many seams certified and how many ranges were redone.
 * --shards N --seamless-dc-agc is the exact --seamless for chains with the DC blocker AND the digital output AGC (--dc-block
 * --agc-profile digital), in the five steps of iqgpu.h's block on such chains.  Shard starts lie on lcm(4096, --chunk-frames), and
 * --chunk-frames is a multiple of the AGC chunk.  Step 1: shards 0 .. N-2 measure the DC maps of every call of their range
 * (iqgpu_chain_dcagc_dc_measure: one row per piece, two for the call the stream cuts at the AGC's lock).  Step 2: one walk over all
 * rows; the state in front of a call is the one in front of its first row.  Step 3: the same shards put their chain at their start
 * with the walked DC state and no AGC entry (iqgpu_chain_dcagc_seek) and measure the AGC rows of their range in shadow calls
 * (iqgpu_chain_dcagc_measure, synchronous).  Step 4: the AGC walk.  Step 5: every shard seeks with both states and runs the usual
 * chunk loop.  The stitched file is the file --shards 1 writes, byte for byte.
 *
 * --synthetic FRAMES [--synthetic-hash SEED]: no input file.  Without a seed one constant pinned buffer is sent again and again
 * (the PCIe-inclusive rate of the path, nothing else); with one, shard s is the stream frame n -> splitmix64((SEED + s) * K + n)
 * of its own (iq_tool_amd/synth.py hash_stream restates it): configs[4] at its real size -- 8 x 2.5 G frames -- without 80 GB of
 * files, every range of every shard reproducible by the checker.  With --seamless the job is ONE stream of seed SEED indexed by the
 * global frame number.
 */
#define _GNU_SOURCE
#define _FILE_OFFSET_BITS 64
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "iqgpu.h"

#define NBUF 2

typedef struct {
    const char *in_path, *out_path;
    iqgpu_chain_desc desc;
    size_t chunk_frames;
    int shards, devices, device0;
    long long synthetic_frames;       /* > 0: no input file, reuse one pinned buffer (PCIe-inclusive rate) */
    int have_hash; unsigned long long hash_seed;   /* ... or generate shard s as the counter-hash stream of seed hash_seed + s */
    int no_bind;                      /* --no-numa-bind */
    int seamless;                     /* --seamless: the shards continue ONE stream (iqgpu_chain_seek behind a preroll) */
    int seamless_agc;                 /* --seamless-agc: --seamless for digital-AGC chains, in two passes (measure, walk, process) */
    int seamless_dc;                  /* --seamless-dc: the exact --seamless for DC-blocker chains, in three passes (measure, walk, process) */
    int seamless_dc_agc;              /* --seamless-dc-agc: exact for chains with the DC blocker and the digital AGC, in five steps */
    int seamless_rms;                 /* --seamless-rms: --seamless for dx / local AGC chains: seek from a bounded window, seams certified, ranges redone where not */
    int have_shards;                  /* --shards was given */
    int dry;                          /* --dry-placement: plan, bind, size the buffers, report -- no GPU call */
    int quiet;
} Options;

typedef struct {
    const Options *opt;
    int shard;
    long long first_frame, frames;    /* input range */
    long long out_offset_bytes;       /* where this shard's output starts in the output file */
    long long frames_out;             /* result */
    long long planned_out;            /* iqgpu_design_out_frames(frames): what out_offset_bytes of the NEXT shard was computed from */
    long long preroll_frames;         /* --seamless: input frames in front of first_frame the chain is warmed up on */
    int device, numa_node;            /* where it ran; -1 = the host does not say / not bound */
    char bus_id[64]; int cpus_allowed; long long pinned_bytes, hbm_bytes;   /* --dry-placement's report */
    double seconds, stream_seconds;   /* whole shard incl. set-up / copy-process-copy loop only */
    /* --seamless-agc */
    iqgpu_agc_chunk *rows; long long agc_rows;   /* pass 1: this shard's table (planned count with --dry-placement) */
    iqgpu_agc_state entry; int have_entry;       /* the AGC state at first_frame, from the walk */
    /* --seamless-dc */
    iqgpu_dc_row *dc_rows; long long n_dc_rows;  /* pass 1: one row per call of this shard's range (planned count with --dry-placement) */
    iqgpu_dc_state dc_entry;                     /* the blocker's state in front of this shard's preroll, from the walk */
    /* --seamless-dc-agc: both of the above, and how many rows every call of the range gave (1 or 2) */
    unsigned char *dc_call_rows; long long n_dc_calls;
    double measure_seconds;
    /* --seamless-rms: the AGC state right after the seek and behind the range, the checkpoint behind the range; redo_blob: this
     * range again from the checkpoint of the range in front (its seam did not certify) */
    iqgpu_agc_state rms_seek_state, rms_end_state;
    void *blob; size_t blob_bytes;
    const void *redo_blob; size_t redo_bytes;
    int certified, redone;
    int barriers;                     /* how many of the rendezvous of the passes (two; --seamless-dc-agc: four) this thread has been through */
    int rc;
    char err[256];
} Shard;

/* --seamless-agc: all shard threads meet behind pass 1 and again behind the walk, which shard 0's thread does in between */
static pthread_barrier_t g_pass;
static Shard *g_shards;
static volatile int g_walk_ok;

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }

/* frame n of the stream with this seed: splitmix64 of a counter (any range of it can be regenerated, iq_tool_amd/synth.py) */
static inline uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* cs16: I, Q = the two low 16-bit words as signed values, arithmetic >> 2 (quarter scale: nothing on the path clips); every other
 * integer format: the low bytes of the hash as they are (full-scale noise) */
static void hash_fill(void *dst, int fmt, size_t bps, uint64_t seed, long long first, size_t n)
{
    const uint64_t base = seed * 0xD1342543DE82EF95ull;
    if (fmt == IQGPU_FMT_CS16) {
        int16_t *d = (int16_t *)dst;
        for (size_t i = 0; i < n; i++) {
            const uint64_t x = mix64(base + (uint64_t)(first + (long long)i));
            d[2 * i] = (int16_t)((int16_t)(x & 0xffffu) >> 2);
            d[2 * i + 1] = (int16_t)((int16_t)((x >> 16) & 0xffffu) >> 2);
        }
    } else {
        unsigned char *d = (unsigned char *)dst;
        for (size_t i = 0; i < n; i++) {
            const uint64_t x = mix64(base + (uint64_t)(first + (long long)i));
            memcpy(d + i * bps, &x, bps);              /* (little-endian hosts only, like the raw formats themselves) */
        }
    }
}

static int fmt_from_name(const char *s)
{
    static const struct { const char *n; int v; } t[] = {
        {"cu8", IQGPU_FMT_CU8}, {"cs8", IQGPU_FMT_CS8}, {"cu16", IQGPU_FMT_CU16}, {"cs16", IQGPU_FMT_CS16},
        {"cs24", IQGPU_FMT_CS24}, {"cu32", IQGPU_FMT_CU32}, {"cs32", IQGPU_FMT_CS32}, {"cf32", IQGPU_FMT_CF32},
        {"sc16q11", IQGPU_FMT_SC16Q11}};
    for (size_t i = 0; i < sizeof(t) / sizeof(t[0]); i++) if (!strcmp(s, t[i].n)) return t[i].v;
    return -1;
}

/* n frames of the job's input from stream frame `first` into dst: the file, the counter-hash stream, or the constant filling */
static int read_frames(const Options *o, int in_fd, int fmt, size_t ibps, long long first, size_t n, void *dst, char *err, size_t errcap)
{
    const size_t nb = n * ibps;
    if (in_fd >= 0) {
        size_t got = 0;
        while (got < nb) {
            ssize_t r = pread(in_fd, (char *)dst + got, nb - got, first * (long long)ibps + (long long)got);
            if (r <= 0) { snprintf(err, errcap, "pread: %s", r < 0 ? strerror(errno) : "short file"); return -1; }
            got += (size_t)r;
        }
    } else if (o->have_hash) hash_fill(dst, fmt, ibps, o->hash_seed, first, n);
    else memset(dst, 0x11, nb);
    return 0;
}

#define CK(call) do { int rc_ = (call); if (rc_ != IQGPU_OK) { snprintf(sh->err, sizeof(sh->err), "%s: %s", #call, iqgpu_last_error()); sh->rc = rc_; goto done; } } while (0)

static void *run_shard(void *arg)
{
    Shard *sh = (Shard *)arg;
    const Options *o = sh->opt;
    iqgpu_chain_desc d = o->desc;
    d.device_ordinal = o->device0 + (sh->shard % o->devices);
    const size_t ibps = iqgpu_get_bytes_per_sample(d.in_format), obps = iqgpu_get_bytes_per_sample(d.out_format);
    iqgpu_chain *chain = NULL;
    void *s_in = NULL, *s_k = NULL, *s_out = NULL;
    void *h_in[NBUF] = {0}, *h_out[NBUF] = {0}, *d_in[NBUF] = {0}, *d_out[NBUF] = {0};
    void *e_in[NBUF] = {0}, *e_k[NBUF] = {0}, *e_out[NBUF] = {0};
    size_t out_frames[NBUF] = {0};
    int in_fd = -1, out_fd = -1;
    void *pre = NULL;
    const double t0 = now_s();

    /* this thread -- and with it the pages it touches first and the buffers it pins -- onto the socket of its GPU, before anything
     * touches that GPU.  Best effort: a host that hides its topology leaves the thread where it is (numa_node stays -1) */
    sh->device = d.device_ordinal; sh->numa_node = -1;
    if (!o->no_bind) { int node = -1; if (iqgpu_bind_thread_to_device(d.device_ordinal, &node) == IQGPU_OK) sh->numa_node = node; }

    if (o->dry) {
        /* --dry-placement: everything the first multi-GPU run does BEFORE its first GPU call -- the device of
         * this shard, its PCI address and NUMA node from sysfs, the binding, the sizes of the buffers it would pin and allocate --
         * and nothing after it.  The capacity rule without a handle: src/pipeline.c:246-258 on the designed ratio */
        int node = -1;
        sh->bus_id[0] = 0;
        (void)iqgpu_device_numa_node(d.device_ordinal, &node, sh->bus_id, sizeof(sh->bus_id));
        if (sh->numa_node < 0 && o->no_bind) sh->numa_node = node;
        { cpu_set_t m; CPU_ZERO(&m); sh->cpus_allowed = pthread_getaffinity_np(pthread_self(), sizeof(m), &m) == 0 ? CPU_COUNT(&m) : -1; }
        size_t cap_frames = 0;
        CK(iqgpu_design_out_frames(&d, o->chunk_frames, &cap_frames));
        cap_frames += 64;
        sh->pinned_bytes = (long long)NBUF * (long long)(o->chunk_frames * ibps + cap_frames * obps);
        sh->hbm_bytes = sh->pinned_bytes;
        sh->frames_out = sh->planned_out;
        goto done;
    }

    CK(iqgpu_chain_create(&d, &chain));
    const size_t chunk = o->chunk_frames;
    const size_t out_cap = iqgpu_chain_max_out_frames(chain, chunk) * obps;
    CK(iqgpu_stream_create(d.device_ordinal, &s_in));
    CK(iqgpu_stream_create(d.device_ordinal, &s_k));
    CK(iqgpu_stream_create(d.device_ordinal, &s_out));
    CK(iqgpu_chain_set_stream(chain, s_k));
    for (int b = 0; b < NBUF; b++) {
        CK(iqgpu_host_malloc_pinned(chunk * ibps, &h_in[b]));
        CK(iqgpu_host_malloc_pinned(out_cap, &h_out[b]));
        CK(iqgpu_device_malloc(d.device_ordinal, chunk * ibps, &d_in[b]));
        CK(iqgpu_device_malloc(d.device_ordinal, out_cap, &d_out[b]));
        CK(iqgpu_event_create(&e_in[b])); CK(iqgpu_event_create(&e_k[b])); CK(iqgpu_event_create(&e_out[b]));
    }
    if (o->synthetic_frames <= 0) {
        in_fd = open(o->in_path, O_RDONLY);
        if (in_fd < 0) { snprintf(sh->err, sizeof(sh->err), "open %s: %s", o->in_path, strerror(errno)); sh->rc = -1; goto done; }
    } else if (!o->have_hash) {
        for (int b = 0; b < NBUF; b++) memset(h_in[b], 0x11 * (b + 1), chunk * ibps);
    }
    if (o->out_path) {
        out_fd = open(o->out_path, O_WRONLY | O_CREAT, 0644);
        if (out_fd < 0) { snprintf(sh->err, sizeof(sh->err), "open %s: %s", o->out_path, strerror(errno)); sh->rc = -1; goto done; }
    }

    if (o->seamless_agc) {
        /* pass 1: the chain at the start of the range with the AGC out of the way, then the range measured in the calls pass 2
         * will make.  The last shard measures nothing: nobody starts behind it */
        const size_t np = (size_t)sh->preroll_frames;
        const size_t agc_chunk = d.agc_chunk_frames ? d.agc_chunk_frames : 16384;
        const double t_m = now_s();
        if (np) {
            pre = malloc(np * ibps);
            if (!pre) { snprintf(sh->err, sizeof(sh->err), "out of memory for a preroll of %zu frames", np); sh->rc = -1; goto done; }
            if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame - sh->preroll_frames, np, pre, sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
        }
        if (sh->shard < o->shards - 1) {
            const size_t cap = (size_t)((sh->frames + (long long)chunk - 1) / (long long)chunk) * ((chunk + agc_chunk - 1) / agc_chunk) + 1;
            /* (pinned: the rows of a batch are copied out asynchronously, behind the kernels of the next one) */
            void *table = NULL;
            if (iqgpu_host_malloc_pinned(cap * sizeof(iqgpu_agc_chunk), &table) != IQGPU_OK) { snprintf(sh->err, sizeof(sh->err), "out of memory for a table of %zu rows", cap); sh->rc = -1; goto done; }
            sh->rows = (iqgpu_agc_chunk *)table;
            CK(iqgpu_chain_seek_agc(chain, (uint64_t)sh->first_frame, pre, np, NULL));
            /* the batch grid and the two pinned input buffers of the ordinary pass below, through the chain's own pipeline: batch i is
             * read while the copy of batch i-1 and the kernels of batch i-2 run; buffer i % 2 is free once batch i-2 is collected */
            uint64_t tk[NBUF] = {0};
            long long i = 0;
            for (long long at = 0; at < sh->frames; at += (long long)chunk, i++) {
                const int b = (int)(i % NBUF);
                size_t n = chunk, got = 0;
                if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
                if (tk[b]) { CK(iqgpu_chain_collect(chain, tk[b])); tk[b] = 0; }
                if (o->synthetic_frames <= 0 || o->have_hash) {
                    if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame + at, n, h_in[b], sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
                }
                CK(iqgpu_chain_measure_submit(chain, h_in[b], n, sh->rows + sh->agc_rows, cap - (size_t)sh->agc_rows, &got, &tk[b]));
                sh->agc_rows += (long long)got;
            }
            for (int b = 0; b < NBUF; b++) if (tk[b]) CK(iqgpu_chain_collect(chain, tk[b]));
        }
        sh->measure_seconds = now_s() - t_m;
        /* the walk: one thread, the tables in shard order, the state in front of every shard kept */
        pthread_barrier_wait(&g_pass); sh->barriers = 1;
        if (sh->shard == 0) {
            int ok = 1;
            iqgpu_agc_state st;
            for (int q = 0; q < o->shards; q++) if (g_shards[q].rc) ok = 0;
            if (ok && iqgpu_chain_agc_initial_state(chain, &st) != IQGPU_OK) ok = 0;
            for (int q = 0; q < o->shards && ok; q++) {
                g_shards[q].entry = st; g_shards[q].have_entry = 1;
                if (q < o->shards - 1 && iqgpu_chain_agc_advance(chain, &st, g_shards[q].rows, (size_t)g_shards[q].agc_rows, NULL) != IQGPU_OK) {
                    snprintf(sh->err, sizeof(sh->err), "iqgpu_chain_agc_advance: %s", iqgpu_last_error()); sh->rc = -1; ok = 0;
                }
            }
            g_walk_ok = ok;
        }
        pthread_barrier_wait(&g_pass); sh->barriers = 2;
        if (!g_walk_ok) { if (!sh->rc) { snprintf(sh->err, sizeof(sh->err), "the measure pass or the walk of another shard failed"); sh->rc = -1; } goto done; }
        /* pass 2: the same position again, now carrying the stream's AGC state there */
        CK(iqgpu_chain_seek_agc(chain, (uint64_t)sh->first_frame, pre, np, &sh->entry));
        free(pre); pre = NULL;
    }
    if (o->seamless_dc) {
        /* pass 1: the map of every call pass 2 will make of this range.  The last shard measures nothing: nobody starts behind it */
        const size_t np = (size_t)sh->preroll_frames;
        const double t_m = now_s();
        if (sh->shard < o->shards - 1) {
            const size_t cap = (size_t)((sh->frames + (long long)chunk - 1) / (long long)chunk);
            sh->dc_rows = (iqgpu_dc_row *)malloc((cap ? cap : 1) * sizeof(iqgpu_dc_row));
            if (!sh->dc_rows) { snprintf(sh->err, sizeof(sh->err), "out of memory for a table of %zu rows", cap); sh->rc = -1; goto done; }
            for (long long at = 0; at < sh->frames; at += (long long)chunk) {
                size_t n = chunk;
                if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
                if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame + at, n, h_in[0], sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
                CK(iqgpu_chain_dc_measure(chain, (uint64_t)(sh->first_frame + at), h_in[0], n, &sh->dc_rows[sh->n_dc_rows]));
                sh->n_dc_rows++;
            }
        }
        sh->measure_seconds = now_s() - t_m;
        /* the walk: one thread, ONE table of all rows in stream order (row k = call k of the single stream), the state in front of
         * every call; every shard then enters its preroll with the state in front of the preroll's first call */
        pthread_barrier_wait(&g_pass); sh->barriers = 1;
        if (sh->shard == 0) {
            int ok = 1;
            long long total = 0;
            for (int q = 0; q < o->shards; q++) { if (g_shards[q].rc) ok = 0; total += g_shards[q].n_dc_rows; }
            iqgpu_dc_row *all = (iqgpu_dc_row *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_row));
            iqgpu_dc_state *before = (iqgpu_dc_state *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_state));
            iqgpu_dc_state st = {0.0, 0.0};
            if (ok && (!all || !before)) { snprintf(sh->err, sizeof(sh->err), "out of memory for the walk over %lld rows", total); sh->rc = -1; ok = 0; }
            if (ok) {
                long long k = 0;
                for (int q = 0; q < o->shards; q++) { if (g_shards[q].n_dc_rows) memcpy(all + k, g_shards[q].dc_rows, (size_t)g_shards[q].n_dc_rows * sizeof(iqgpu_dc_row)); k += g_shards[q].n_dc_rows; }
                if (iqgpu_chain_dc_advance(chain, &st, all, (size_t)total, before) != IQGPU_OK) {
                    snprintf(sh->err, sizeof(sh->err), "iqgpu_chain_dc_advance: %s", iqgpu_last_error()); sh->rc = -1; ok = 0;
                }
            }
            for (int q = 1; q < o->shards && ok; q++) {
                const long long k = (g_shards[q].first_frame - g_shards[q].preroll_frames) / (long long)chunk;
                /* (k == total: a preroll of no frames in front of the last shard -- a chain without filter memory; the state behind the last row) */
                if (k < 0 || k > total) { snprintf(sh->err, sizeof(sh->err), "the walk holds no state in front of call %lld", k); sh->rc = -1; ok = 0; break; }
                g_shards[q].dc_entry = k < total ? before[k] : st;
            }
            free(all); free(before);
            g_walk_ok = ok;
        }
        pthread_barrier_wait(&g_pass); sh->barriers = 2;
        if (!g_walk_ok) { if (!sh->rc) { snprintf(sh->err, sizeof(sh->err), "the measure pass or the walk of another shard failed"); sh->rc = -1; } goto done; }
        /* pass 2: the chain at the start of the range, behind a preroll of whole calls entered with the walked state */
        if (sh->first_frame > 0) {
            pre = malloc(np ? np * ibps : 1);
            if (!pre) { snprintf(sh->err, sizeof(sh->err), "out of memory for a preroll of %zu frames", np); sh->rc = -1; goto done; }
            if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame - sh->preroll_frames, np, pre, sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
            CK(iqgpu_chain_seek_dc(chain, (uint64_t)sh->first_frame, pre, np, chunk, &sh->dc_entry));
            free(pre); pre = NULL;
        }
    }
    if (o->seamless_dc_agc) {
        const size_t np = (size_t)sh->preroll_frames;
        const size_t agc_chunk = d.agc_chunk_frames ? d.agc_chunk_frames : 16384;
        const size_t calls = (size_t)((sh->frames + (long long)chunk - 1) / (long long)chunk);
        const int measures = sh->shard < o->shards - 1;     /* the last shard measures nothing: nobody starts behind it */
        const double t_m = now_s();
        /* step 1: the DC maps of every call step 5 will make of this range, one row per piece */
        if (measures) {
            sh->dc_rows = (iqgpu_dc_row *)malloc((2 * calls + 1) * sizeof(iqgpu_dc_row));
            sh->dc_call_rows = (unsigned char *)malloc(calls + 1);
            if (!sh->dc_rows || !sh->dc_call_rows) { snprintf(sh->err, sizeof(sh->err), "out of memory for a table of %zu rows", 2 * calls); sh->rc = -1; goto done; }
            for (long long at = 0; at < sh->frames; at += (long long)chunk) {
                size_t n = chunk, got = 0;
                if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
                if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame + at, n, h_in[0], sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
                CK(iqgpu_chain_dcagc_dc_measure(chain, (uint64_t)(sh->first_frame + at), h_in[0], n, &sh->dc_rows[sh->n_dc_rows], 2, &got));
                sh->dc_call_rows[sh->n_dc_calls++] = (unsigned char)got;
                sh->n_dc_rows += (long long)got;
            }
        }
        /* step 2: one thread walks ALL rows in stream order; the state in front of grid call k stands in front of its first row */
        pthread_barrier_wait(&g_pass); sh->barriers = 1;
        if (sh->shard == 0) {
            int ok = 1;
            long long total = 0, total_calls = 0;
            for (int q = 0; q < o->shards; q++) { if (g_shards[q].rc) ok = 0; total += g_shards[q].n_dc_rows; total_calls += g_shards[q].n_dc_calls; }
            iqgpu_dc_row *all = (iqgpu_dc_row *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_row));
            iqgpu_dc_state *before = (iqgpu_dc_state *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_state));
            long long *first_row = (long long *)malloc((size_t)(total_calls + 1) * sizeof(long long));
            iqgpu_dc_state st = {0.0, 0.0};
            if (ok && (!all || !before || !first_row)) { snprintf(sh->err, sizeof(sh->err), "out of memory for the walk over %lld rows", total); sh->rc = -1; ok = 0; }
            if (ok) {
                long long k = 0, call = 0;
                for (int q = 0; q < o->shards; q++) {
                    if (g_shards[q].n_dc_rows) memcpy(all + k, g_shards[q].dc_rows, (size_t)g_shards[q].n_dc_rows * sizeof(iqgpu_dc_row));
                    long long r = k;
                    for (long long j = 0; j < g_shards[q].n_dc_calls; j++) { first_row[call++] = r; r += g_shards[q].dc_call_rows[j]; }
                    k += g_shards[q].n_dc_rows;
                }
                first_row[call] = k;
                if (iqgpu_chain_dcagc_dc_advance(chain, &st, all, (size_t)total, before) != IQGPU_OK) {
                    snprintf(sh->err, sizeof(sh->err), "iqgpu_chain_dcagc_dc_advance: %s", iqgpu_last_error()); sh->rc = -1; ok = 0;
                }
            }
            for (int q = 1; q < o->shards && ok; q++) {
                const long long k = (g_shards[q].first_frame - g_shards[q].preroll_frames) / (long long)chunk;
                if (k < 0 || k > total_calls) { snprintf(sh->err, sizeof(sh->err), "the walk holds no state in front of call %lld", k); sh->rc = -1; ok = 0; break; }
                g_shards[q].dc_entry = first_row[k] < total ? before[first_row[k]] : st;
            }
            free(all); free(before); free(first_row);
            g_walk_ok = ok;
        }
        pthread_barrier_wait(&g_pass); sh->barriers = 2;
        if (!g_walk_ok) { if (!sh->rc) { snprintf(sh->err, sizeof(sh->err), "the DC measure pass or the walk of another shard failed"); sh->rc = -1; } goto done; }
        /* step 3: the chain at the start of the range -- the preroll as shadow calls from the walked DC state, no AGC entry -- and the
         * AGC rows of every call of the range, as shadow calls (synchronous: the pipelined measure makes no shadow calls) */
        if (np) {
            pre = malloc(np * ibps);
            if (!pre) { snprintf(sh->err, sizeof(sh->err), "out of memory for a preroll of %zu frames", np); sh->rc = -1; goto done; }
            if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame - sh->preroll_frames, np, pre, sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
        }
        if (measures) {
            const size_t cap = calls * ((chunk + agc_chunk - 1) / agc_chunk) + 1;
            void *table = NULL;
            if (iqgpu_host_malloc_pinned(cap * sizeof(iqgpu_agc_chunk), &table) != IQGPU_OK) { snprintf(sh->err, sizeof(sh->err), "out of memory for a table of %zu rows", cap); sh->rc = -1; goto done; }
            sh->rows = (iqgpu_agc_chunk *)table;
            CK(iqgpu_chain_dcagc_seek(chain, (uint64_t)sh->first_frame, pre, np, chunk, &sh->dc_entry, NULL));
            for (long long at = 0; at < sh->frames; at += (long long)chunk) {
                size_t n = chunk, got = 0;
                if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
                if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame + at, n, h_in[0], sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
                CK(iqgpu_chain_dcagc_measure(chain, h_in[0], n, sh->rows + sh->agc_rows, cap - (size_t)sh->agc_rows, &got));
                sh->agc_rows += (long long)got;
            }
        }
        sh->measure_seconds = now_s() - t_m;
        /* step 4: the AGC walk, the tables in shard order */
        pthread_barrier_wait(&g_pass); sh->barriers = 3;
        if (sh->shard == 0) {
            int ok = 1;
            iqgpu_agc_state st;
            for (int q = 0; q < o->shards; q++) if (g_shards[q].rc) ok = 0;
            if (ok && iqgpu_chain_agc_initial_state(chain, &st) != IQGPU_OK) ok = 0;
            for (int q = 0; q < o->shards && ok; q++) {
                g_shards[q].entry = st; g_shards[q].have_entry = 1;
                if (q < o->shards - 1 && iqgpu_chain_agc_advance(chain, &st, g_shards[q].rows, (size_t)g_shards[q].agc_rows, NULL) != IQGPU_OK) {
                    snprintf(sh->err, sizeof(sh->err), "iqgpu_chain_agc_advance: %s", iqgpu_last_error()); sh->rc = -1; ok = 0;
                }
            }
            g_walk_ok = ok;
        }
        pthread_barrier_wait(&g_pass); sh->barriers = 4;
        if (!g_walk_ok) { if (!sh->rc) { snprintf(sh->err, sizeof(sh->err), "the AGC measure pass or the walk of another shard failed"); sh->rc = -1; } goto done; }
        /* step 5: the same position again, now with both states of the stream there */
        CK(iqgpu_chain_dcagc_seek(chain, (uint64_t)sh->first_frame, pre, np, chunk, &sh->dc_entry, &sh->entry));
        free(pre); pre = NULL;
    }
    if (o->seamless_rms && sh->redo_blob) {
        /* the seam in front of this range did not certify: the range again, from where the range in front really ended */
        CK(iqgpu_chain_load_state(chain, sh->redo_blob, sh->redo_bytes));
    } else if (o->seamless_rms && sh->first_frame > 0) {
        const size_t np = (size_t)sh->preroll_frames;
        pre = malloc(np ? np * ibps : 1);
        if (!pre) { snprintf(sh->err, sizeof(sh->err), "out of memory for a preroll of %zu frames", np); sh->rc = -1; goto done; }
        if (read_frames(o, in_fd, d.in_format, ibps, sh->first_frame - sh->preroll_frames, np, pre, sh->err, sizeof(sh->err))) { sh->rc = -1; goto done; }
        CK(iqgpu_chain_seek_rms(chain, (uint64_t)sh->first_frame, pre, np));
        CK(iqgpu_chain_get_agc_state(chain, &sh->rms_seek_state));
        free(pre); pre = NULL;
    }
    if (o->seamless && sh->first_frame > 0) {
        /* the frames in front of this shard's start, read like any other range of the stream, warm the chain's histories up; the
         * chain then stands at first_frame of the ONE stream (iqgpu_chain_seek) */
        const size_t np = (size_t)sh->preroll_frames, nb = np * ibps;
        const long long from = sh->first_frame - sh->preroll_frames;
        pre = malloc(nb ? nb : 1);
        if (!pre) { snprintf(sh->err, sizeof(sh->err), "out of memory for a preroll of %zu frames", np); sh->rc = -1; goto done; }
        if (in_fd >= 0) {
            size_t got = 0;
            while (got < nb) {
                ssize_t r = pread(in_fd, (char *)pre + got, nb - got, from * (long long)ibps + (long long)got);
                if (r <= 0) { snprintf(sh->err, sizeof(sh->err), "pread: %s", r < 0 ? strerror(errno) : "short file"); sh->rc = -1; goto done; }
                got += (size_t)r;
            }
        } else if (o->have_hash) hash_fill(pre, d.in_format, ibps, o->hash_seed, from, np);
        else memset(pre, 0x11, nb);
        CK(iqgpu_chain_seek(chain, (uint64_t)sh->first_frame, pre, np));
        free(pre); pre = NULL;
    }

    long long done_in = 0, written = 0;
    const double t_loop = now_s();
    long long n_chunks = (sh->frames + (long long)chunk - 1) / (long long)chunk;
    /* software pipeline: iteration i first issues chunk i (H2D, kernels, D2H, all asynchronous), then
     * retires chunk i-1 (waits for its D2H, writes it): chunk i's copies and kernels overlap the
     * write-out of chunk i-1, and buffer i % 2 is free again because chunk i-2 retired last time */
    for (long long i = 0; i <= n_chunks; i++) {
        if (i < n_chunks) {
            const int b = (int)(i % NBUF);
            size_t n = chunk;
            if ((long long)n > sh->frames - done_in) n = (size_t)(sh->frames - done_in);
            if (in_fd >= 0) {
                const size_t nb = n * ibps;
                size_t got = 0;
                while (got < nb) {
                    ssize_t r = pread(in_fd, (char *)h_in[b] + got, nb - got, (sh->first_frame + done_in) * (long long)ibps + (long long)got);
                    if (r <= 0) { snprintf(sh->err, sizeof(sh->err), "pread: %s", r < 0 ? strerror(errno) : "short file"); sh->rc = -1; goto done; }
                    got += (size_t)r;
                }
            } else if (o->have_hash) {
                /* (buffer b is free: chunk i - 2, its last user, retired in the iteration before this one) */
                if (o->seamless || o->seamless_agc || o->seamless_dc || o->seamless_dc_agc || o->seamless_rms) hash_fill(h_in[b], d.in_format, ibps, o->hash_seed, sh->first_frame + done_in, n);
                else hash_fill(h_in[b], d.in_format, ibps, o->hash_seed + (uint64_t)sh->shard, done_in, n);
            }
            CK(iqgpu_memcpy_h2d_async(d_in[b], h_in[b], n * ibps, s_in));
            CK(iqgpu_event_record(e_in[b], s_in));
            CK(iqgpu_stream_wait_event(s_k, e_in[b]));
            CK(iqgpu_chain_process_device(chain, d_in[b], n, d_out[b], out_cap, &out_frames[b]));
            CK(iqgpu_event_record(e_k[b], s_k));
            CK(iqgpu_stream_wait_event(s_out, e_k[b]));
            if (out_frames[b]) CK(iqgpu_memcpy_d2h_async(h_out[b], d_out[b], out_frames[b] * obps, s_out));
            CK(iqgpu_event_record(e_out[b], s_out));
            done_in += (long long)n;
        }
        if (i >= 1) {
            const int b = (int)((i - 1) % NBUF);
            float ms;
            CK(iqgpu_event_elapsed_ms(e_k[b], e_out[b], &ms));    /* synchronises on e_out */
            if (out_fd >= 0 && out_frames[b]) {
                const size_t nb = out_frames[b] * obps;
                if (pwrite(out_fd, h_out[b], nb, sh->out_offset_bytes + written * (long long)obps) != (ssize_t)nb) {
                    snprintf(sh->err, sizeof(sh->err), "pwrite: %s", strerror(errno)); sh->rc = -1; goto done;
                }
            }
            written += (long long)out_frames[b];
        }
    }
    sh->frames_out = written;
    sh->stream_seconds = now_s() - t_loop;
    if (written != sh->planned_out) {
        snprintf(sh->err, sizeof(sh->err), "shard %d produced %lld frames, its place in the output was planned for %lld", sh->shard, written, sh->planned_out);
        sh->rc = -1;
    }
    if (o->seamless_rms && !sh->rc) {
        /* what the seam behind this range is checked against, and what the range behind it restarts from if the check fails */
        size_t need = 0;
        CK(iqgpu_chain_get_agc_state(chain, &sh->rms_end_state));
        (void)iqgpu_chain_save_state(chain, NULL, 0, &need);          /* (a size query: IQGPU_ECAPACITY) */
        free(sh->blob);
        sh->blob = malloc(need ? need : 1);
        if (!sh->blob) { snprintf(sh->err, sizeof(sh->err), "out of memory for a checkpoint of %zu bytes", need); sh->rc = -1; goto done; }
        CK(iqgpu_chain_save_state(chain, sh->blob, need, &sh->blob_bytes));
    }
done:
    /* (a shard that fails early still keeps the rendezvous of the two passes: the others wait there) */
    while ((o->seamless_agc || o->seamless_dc || o->seamless_dc_agc) && !o->dry && sh->barriers < (o->seamless_dc_agc ? 4 : 2)) { pthread_barrier_wait(&g_pass); sh->barriers++; }
    free(pre);
    if (chain) iqgpu_chain_synchronize(chain);
    for (int b = 0; b < NBUF; b++) {
        if (e_in[b]) iqgpu_event_destroy(e_in[b]);
        if (e_k[b]) iqgpu_event_destroy(e_k[b]);
        if (e_out[b]) iqgpu_event_destroy(e_out[b]);
        if (h_in[b]) iqgpu_host_free_pinned(h_in[b]);
        if (h_out[b]) iqgpu_host_free_pinned(h_out[b]);
        if (d_in[b]) iqgpu_device_free(d.device_ordinal, d_in[b]);
        if (d_out[b]) iqgpu_device_free(d.device_ordinal, d_out[b]);
    }
    if (s_in) iqgpu_stream_destroy(s_in);
    if (s_k) { if (chain) iqgpu_chain_set_stream(chain, NULL); iqgpu_stream_destroy(s_k); }
    if (s_out) iqgpu_stream_destroy(s_out);
    if (chain) iqgpu_chain_destroy(chain);
    if (in_fd >= 0) close(in_fd);
    if (out_fd >= 0) close(out_fd);
    sh->seconds = now_s() - t0;
    return NULL;
}

static void usage(void)
{
    fprintf(stderr,
            "iqgpu_run -i IN --raw-file-input-rate HZ --raw-file-input-sample-format FMT -o OUT --output-rate HZ\n"
            "          [--output-sample-format FMT] [--freq-shift HZ] [--shift-after-resample] [--gain G] [--dc-block]\n"
            "          [--iq-factors MAG:PHASE] [--no-resample] [--lowpass HZ] [--highpass HZ] [--pass-range A:B] [--stopband A:B]\n"
            "          [--transition-width HZ] [--attenuation DB] [--filter-taps N] [--filter-type fir|fft] [--filter-fft-size N]\n"
            "          [--chunk-frames N (default 4194304)] [--shards N] [--devices N] [--device D] [--synthetic FRAMES [--synthetic-hash SEED]]\n"
            "          [--seamless (with --shards: the shards continue ONE stream -- the stitched output is what --shards 1 writes)]\n"
            "          [--seamless-agc (--seamless for chains with the digital output AGC: a measure pass, one walk, then the ordinary pass)]\n"
            "          [--seamless-dc (the exact --seamless for --dc-block chains without an AGC: a measure pass over the input, one walk, then the ordinary pass)]\n"
            "          [--seamless-rms (--seamless for chains with the dx / local output AGC: seek from a bounded window, seams certified, a range behind a seam that is not is redone)]\n"
            "          [--seamless-dc-agc (the exact --seamless for --dc-block chains with the digital AGC: DC measure, walk, shadow AGC measure, walk, then the ordinary pass)]\n"
            "          [--no-numa-bind] [--quiet] [--debug NAME=VALUE (iqgpu_debug_set)]\n"
            "          [--dry-placement (plan the shards, bind every shard thread, size its buffers, report as JSON: no GPU call)]\n");
}

int main(int argc, char **argv)
{
    Options o;
    memset(&o, 0, sizeof(o));
    iqgpu_chain_desc_init(&o.desc);
    o.chunk_frames = 1u << 22; o.shards = 1; o.devices = 1;
    double in_rate = 0, out_rate = 0;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
#define NEXT (i + 1 < argc ? argv[++i] : (usage(), exit(2), ""))
        if (!strcmp(a, "-i") || !strcmp(a, "--input")) { const char *v = NEXT; if (!strcmp(v, "raw-file")) v = NEXT; o.in_path = v; }
        else if (!strcmp(a, "-o") || !strcmp(a, "--output")) { const char *v = NEXT; if (!strcmp(v, "raw-file")) v = NEXT; o.out_path = v; }
        else if (!strcmp(a, "--raw-file-input-rate")) in_rate = atof(NEXT);
        else if (!strcmp(a, "--raw-file-input-sample-format")) o.desc.in_format = fmt_from_name(NEXT);
        else if (!strcmp(a, "--output-rate")) out_rate = atof(NEXT);
        else if (!strcmp(a, "--output-sample-format")) o.desc.out_format = fmt_from_name(NEXT);
        else if (!strcmp(a, "--freq-shift")) o.desc.shift_hz = atof(NEXT);
        else if (!strcmp(a, "--shift-after-resample")) o.desc.shift_after_resample = 1;
        else if (!strcmp(a, "--gain")) o.desc.gain = (float)atof(NEXT);
        else if (!strcmp(a, "--dc-block")) o.desc.dc_block_enable = 1;
        else if (!strcmp(a, "--iq-factors")) { o.desc.iq_correct_enable = 1; sscanf(NEXT, "%f:%f", &o.desc.iq_mag, &o.desc.iq_phase); }
        else if (!strcmp(a, "--no-resample")) o.desc.no_resample = 1;
        else if (!strcmp(a, "--lowpass") || !strcmp(a, "--highpass")) {
            if (o.desc.n_filters >= 5) { fprintf(stderr, "at most 5 filters\n"); return 2; }
            iqgpu_filter_req *r = &o.desc.filters[o.desc.n_filters++];
            r->type = !strcmp(a, "--lowpass") ? IQGPU_FILTER_LOWPASS : IQGPU_FILTER_HIGHPASS; r->f1_hz = (float)atof(NEXT); r->f2_hz = 0;
        } else if (!strcmp(a, "--pass-range") || !strcmp(a, "--stopband")) {
            if (o.desc.n_filters >= 5) { fprintf(stderr, "at most 5 filters\n"); return 2; }
            float s = 0, e = 0; sscanf(NEXT, "%f:%f", &s, &e);
            iqgpu_filter_req *r = &o.desc.filters[o.desc.n_filters++];
            r->type = !strcmp(a, "--pass-range") ? IQGPU_FILTER_PASSBAND : IQGPU_FILTER_STOPBAND;
            const float bw = e - s; r->f1_hz = s + (bw / 2.0f); r->f2_hz = bw;     /* src/config.c:203-214 */
        }
        else if (!strcmp(a, "--transition-width")) o.desc.transition_width_hz = (float)atof(NEXT);
        else if (!strcmp(a, "--attenuation")) o.desc.attenuation_db = (float)atof(NEXT);
        else if (!strcmp(a, "--filter-taps")) { int t = atoi(NEXT); if (t && t % 2 == 0) t++; o.desc.filter_taps = t; }   /* src/config.c:233-236 */
        else if (!strcmp(a, "--filter-type")) { const char *v = NEXT; o.desc.filter_impl = !strcmp(v, "fft") ? IQGPU_FILTER_IMPL_FFT : IQGPU_FILTER_IMPL_FIR; }
        else if (!strcmp(a, "--filter-fft-size")) o.desc.fft_size = atoi(NEXT);
        else if (!strcmp(a, "--output-agc")) { o.desc.agc_enable = 1; if (!o.desc.agc_profile) o.desc.agc_profile = IQGPU_AGC_LOCAL; }   /* src/config.c:306-310 */
        else if (!strcmp(a, "--agc-profile")) { const char *v = NEXT; o.desc.agc_enable = 1;
            o.desc.agc_profile = !strcasecmp(v, "dx") ? IQGPU_AGC_DX : !strcasecmp(v, "local") ? IQGPU_AGC_LOCAL : !strcasecmp(v, "digital") ? IQGPU_AGC_DIGITAL : -1; }
        else if (!strcmp(a, "--agc-target")) o.desc.agc_target = (float)atof(NEXT);
        else if (!strcmp(a, "--chunk-frames")) o.chunk_frames = (size_t)atoll(NEXT);
        else if (!strcmp(a, "--shards")) { o.shards = atoi(NEXT); o.have_shards = 1; }
        else if (!strcmp(a, "--devices")) o.devices = atoi(NEXT);
        else if (!strcmp(a, "--device")) o.device0 = atoi(NEXT);
        else if (!strcmp(a, "--synthetic")) o.synthetic_frames = atoll(NEXT);
        else if (!strcmp(a, "--synthetic-hash")) { o.have_hash = 1; o.hash_seed = strtoull(NEXT, NULL, 0); }
        else if (!strcmp(a, "--no-numa-bind")) o.no_bind = 1;
        else if (!strcmp(a, "--dry-placement")) o.dry = 1;
        else if (!strcmp(a, "--seamless")) o.seamless = 1;
        else if (!strcmp(a, "--seamless-agc")) o.seamless_agc = 1;
        else if (!strcmp(a, "--seamless-dc")) o.seamless_dc = 1;
        else if (!strcmp(a, "--seamless-dc-agc")) o.seamless_dc_agc = 1;
        else if (!strcmp(a, "--seamless-rms")) o.seamless_rms = 1;
        else if (!strcmp(a, "--debug")) {              /* --debug name=value -> iqgpu_debug_set (the library reads no environment) */
            char kv[512]; snprintf(kv, sizeof(kv), "%s", NEXT);
            char *eq = strchr(kv, '=');
            if (!eq) { fprintf(stderr, "--debug wants name=value\n"); return 2; }
            *eq = 0;
            if (iqgpu_debug_set(kv, eq + 1) != IQGPU_OK) { fprintf(stderr, "%s\n", iqgpu_last_error()); return 2; }
        }
        else if (!strcmp(a, "--quiet")) o.quiet = 1;
        else { usage(); return 2; }
    }
    if (o.desc.in_format < 0 || o.desc.out_format < 0) { fprintf(stderr, "unknown sample format\n"); return 2; }
    if (o.have_hash && (o.synthetic_frames <= 0 || o.desc.in_format == IQGPU_FMT_CF32)) { fprintf(stderr, "--synthetic-hash needs --synthetic FRAMES and an integer input format\n"); return 2; }
    if (!(in_rate > 0) || (!o.desc.no_resample && !(out_rate > 0)) || (!o.in_path && o.synthetic_frames <= 0)) { usage(); return 2; }
    o.desc.input_rate_hz = in_rate; o.desc.target_rate_hz = o.desc.no_resample ? in_rate : out_rate;
    if (o.shards < 1) o.shards = 1;
    if (o.devices < 1) o.devices = 1;
    if (o.seamless_rms) {
        if (o.seamless || o.seamless_agc || o.seamless_dc || o.seamless_dc_agc) { fprintf(stderr, "--seamless-rms excludes the other --seamless modes\n"); return 2; }
        if (!o.have_shards) { fprintf(stderr, "--seamless-rms needs --shards N\n"); return 2; }
        if (o.synthetic_frames > 0 && !o.have_hash) { fprintf(stderr, "--seamless-rms needs a stream it can read twice: an input file, or --synthetic with --synthetic-hash\n"); return 2; }
        if (o.chunk_frames == 0) { fprintf(stderr, "--seamless-rms: --chunk-frames 0\n"); return 2; }
    }
    if (o.seamless_dc_agc) {
        if (o.seamless || o.seamless_agc || o.seamless_dc) { fprintf(stderr, "--seamless-dc-agc excludes --seamless, --seamless-agc and --seamless-dc\n"); return 2; }
        if (!o.have_shards) { fprintf(stderr, "--seamless-dc-agc needs --shards N\n"); return 2; }
        if (!o.desc.dc_block_enable) { fprintf(stderr, "--seamless-dc-agc: the chain has no DC blocker: give --dc-block, or use --seamless-agc\n"); return 1; }
        if (!o.desc.agc_enable) { fprintf(stderr, "--seamless-dc-agc: the chain has no output AGC (use --seamless-dc)\n"); return 1; }
        if (o.desc.agc_profile != IQGPU_AGC_DIGITAL) {
            fprintf(stderr, "--seamless-dc-agc: the AGC profiles dx / local carry a per-sample loop state that no table of per-chunk figures reproduces exactly; "
                            "only the digital profile is sharded seamlessly\n");
            return 1;
        }
        if (o.synthetic_frames > 0 && !o.have_hash) { fprintf(stderr, "--seamless-dc-agc needs a stream it can read twice: an input file, or --synthetic with --synthetic-hash\n"); return 2; }
        const size_t agc_chunk = o.desc.agc_chunk_frames ? o.desc.agc_chunk_frames : 16384;
        if (o.chunk_frames == 0 || o.chunk_frames % agc_chunk) { fprintf(stderr, "--seamless-dc-agc: --chunk-frames has to be a multiple of the AGC chunk (%zu frames)\n", agc_chunk); return 2; }
    }
    if (o.seamless_dc) {
        /* options that do not go together: exit status 2, as for every other misuse of the command line.  A chain the recipe does not
         * cover -- what the library would refuse at its first call -- : exit status 1, before anything is planned */
        if (o.seamless || o.seamless_agc) { fprintf(stderr, "--seamless-dc excludes --seamless and --seamless-agc\n"); return 2; }
        if (!o.have_shards) { fprintf(stderr, "--seamless-dc needs --shards N\n"); return 2; }
        if (o.desc.agc_enable) { fprintf(stderr, "--seamless-dc: a chain with the output AGC is not covered (its measure route may cut a call into other segments "
                                                 "than its process route)%s\n", o.desc.agc_profile == IQGPU_AGC_DIGITAL ? "; --seamless-agc shards it to the DC bound" : ""); return 1; }
        if (!o.desc.dc_block_enable) { fprintf(stderr, "--seamless-dc: the chain has no DC blocker: give --dc-block, or use --seamless\n"); return 1; }
        if (o.synthetic_frames > 0 && !o.have_hash) { fprintf(stderr, "--seamless-dc needs a stream it can read twice: an input file, or --synthetic with --synthetic-hash\n"); return 2; }
        if (o.chunk_frames == 0) { fprintf(stderr, "--seamless-dc: --chunk-frames 0\n"); return 2; }
    }

    const size_t ibps = iqgpu_get_bytes_per_sample(o.desc.in_format), obps = iqgpu_get_bytes_per_sample(o.desc.out_format);
    long long total_frames = o.synthetic_frames;
    if (total_frames <= 0) {
        struct stat st;
        if (stat(o.in_path, &st) != 0) { fprintf(stderr, "stat %s: %s\n", o.in_path, strerror(errno)); return 1; }
        total_frames = (long long)(st.st_size / (off_t)ibps);
    }
    /* shard plan: equal frame ranges (the last takes the rest), output offsets from the closed form */
    Shard *sh = (Shard *)calloc((size_t)o.shards, sizeof(Shard));
    iqgpu_chain_info info;
    {
        int rc = iqgpu_design_probe(&o.desc, &info, NULL, 0, NULL, 0, NULL, 0);
        if (rc != IQGPU_OK) { fprintf(stderr, "%s\n", iqgpu_last_error()); return 1; }
    }
    long long per = total_frames / o.shards, off = 0;
    uint64_t preroll = 0;
    if (o.seamless && iqgpu_design_preroll_frames(&o.desc, &preroll) != IQGPU_OK) { fprintf(stderr, "--seamless: %s\n", iqgpu_last_error()); return 1; }
    for (int s = 0; s < o.shards && o.seamless; s++) {
        /* ONE stream cut at multiples of 4096 frames (the last shard takes the rest): place and count from the stream's closed form */
        const long long next = (s == o.shards - 1) ? total_frames : ((long long)(s + 1) * per) & ~4095ll;
        sh[s].opt = &o; sh[s].shard = s;
        sh[s].first_frame = ((long long)s * per) & ~4095ll;
        sh[s].frames = next - sh[s].first_frame;
        sh[s].preroll_frames = sh[s].first_frame < (long long)preroll ? sh[s].first_frame : (long long)preroll;
        uint64_t first_out = 0, nout = 0;
        if (iqgpu_design_out_frames_range(&o.desc, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) {
            fprintf(stderr, "%s\n", iqgpu_last_error()); return 1;
        }
        sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
        sh[s].planned_out = (long long)nout;
    }
    if (o.seamless_rms) {
        /* a chain the seek refuses is refused here, in the library's words; placement does not depend on the AGC */
        if (iqgpu_design_preroll_frames_rms(&o.desc, &preroll) != IQGPU_OK) { fprintf(stderr, "--seamless-rms: %s\n", iqgpu_last_error()); return 1; }
        iqgpu_chain_desc na = o.desc;
        na.agc_enable = 0;
        for (int s = 0; s < o.shards; s++) {
            const long long next = (s == o.shards - 1) ? total_frames : ((long long)(s + 1) * per) & ~4095ll;
            sh[s].opt = &o; sh[s].shard = s;
            sh[s].first_frame = ((long long)s * per) & ~4095ll;
            sh[s].frames = next - sh[s].first_frame;
            if (sh[s].frames <= 0) {
                fprintf(stderr, "--seamless-rms: %lld frames are too few for %d shards on a grid of 4096 frames: shard %d would be empty\n", total_frames, o.shards, s);
                return 1;
            }
            sh[s].preroll_frames = sh[s].first_frame < (long long)preroll ? sh[s].first_frame : (long long)preroll;
            uint64_t first_out = 0, nout = 0;
            if (iqgpu_design_out_frames_range(&na, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) {
                fprintf(stderr, "%s\n", iqgpu_last_error()); return 1;
            }
            sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
            sh[s].planned_out = (long long)nout;
        }
    }
    if (o.seamless_agc) {
        /* what the library would refuse at the first v8 call, before anything is planned (its own words) */
        if (o.seamless) { fprintf(stderr, "--seamless and --seamless-agc exclude each other\n"); return 2; }
        if (!o.desc.agc_enable) { fprintf(stderr, "--seamless-agc: the chain has no output AGC (use --seamless)\n"); return 1; }
        /* the two passes have to read the SAME stream: the constant filling of a bare --synthetic is no stream (its buffers differ) */
        if (o.synthetic_frames > 0 && !o.have_hash) { fprintf(stderr, "--seamless-agc needs a stream it can read twice: an input file, or --synthetic with --synthetic-hash\n"); return 2; }
        if (o.desc.agc_profile != IQGPU_AGC_DIGITAL) {
            fprintf(stderr, "--seamless-agc: the AGC profiles dx / local carry a per-sample loop state that no table of per-chunk figures reproduces exactly; "
                            "only the digital profile is sharded seamlessly\n");
            return 1;
        }
        /* preroll and placement do not depend on the AGC: from the description with the AGC off (iqgpu.h) */
        iqgpu_chain_desc na = o.desc;
        na.agc_enable = 0;
        if (iqgpu_design_preroll_frames(&na, &preroll) != IQGPU_OK) { fprintf(stderr, "--seamless-agc: %s\n", iqgpu_last_error()); return 1; }
        /* cut points: multiples of lcm(4096, AGC chunk, --chunk-frames) */
        long long grid = 4096, agc_chunk = o.desc.agc_chunk_frames ? (long long)o.desc.agc_chunk_frames : 16384;
        const long long parts[2] = {agc_chunk, (long long)o.chunk_frames};
        for (int k = 0; k < 2; k++) { long long x = grid, y = parts[k]; while (y) { const long long t = x % y; x = y; y = t; } grid = grid / x * parts[k]; }
        for (int s = 0; s < o.shards; s++) {
            const long long next = (s == o.shards - 1) ? total_frames : ((long long)(s + 1) * per) / grid * grid;
            sh[s].opt = &o; sh[s].shard = s;
            sh[s].first_frame = ((long long)s * per) / grid * grid;
            sh[s].frames = next - sh[s].first_frame;
            if (sh[s].frames <= 0) {
                fprintf(stderr, "--seamless-agc: %lld frames are too few for %d shards on a grid of %lld frames (lcm of 4096, the AGC chunk and --chunk-frames): "
                                "shard %d would be empty\n", total_frames, o.shards, grid, s);
                return 1;
            }
            sh[s].preroll_frames = sh[s].first_frame < (long long)preroll ? sh[s].first_frame : (long long)preroll;
            uint64_t first_out = 0, nout = 0;
            if (iqgpu_design_out_frames_range(&na, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) {
                fprintf(stderr, "%s\n", iqgpu_last_error()); return 1;
            }
            sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
            sh[s].planned_out = (long long)nout;
            if (o.dry && s < o.shards - 1) {        /* rows pass 1 will record: one per AGC chunk of every call */
                const long long cf = (long long)o.chunk_frames, full = sh[s].frames / cf, rest = sh[s].frames % cf;
                sh[s].agc_rows = full * ((cf + agc_chunk - 1) / agc_chunk) + (rest + agc_chunk - 1) / agc_chunk;
            }
        }
        g_shards = sh;
        if (!o.dry && pthread_barrier_init(&g_pass, NULL, (unsigned)o.shards) != 0) { fprintf(stderr, "pthread_barrier_init failed\n"); return 1; }
    }
    if (o.seamless_dc) {
        /* the preroll is the filters' memory alone -- the description with the blocker off -- in whole calls; placement does not depend
         * on the blocker */
        iqgpu_chain_desc nd = o.desc;
        nd.dc_block_enable = 0;
        if (iqgpu_design_preroll_frames(&nd, &preroll) != IQGPU_OK) { fprintf(stderr, "--seamless-dc: %s\n", iqgpu_last_error()); return 1; }
        const long long cf = (long long)o.chunk_frames;
        const long long pre_calls = ((long long)preroll + cf - 1) / cf * cf;
        long long grid = 4096;
        { long long x = grid, y = cf; while (y) { const long long t = x % y; x = y; y = t; } grid = grid / x * cf; }
        for (int s = 0; s < o.shards; s++) {
            const long long next = (s == o.shards - 1) ? total_frames : ((long long)(s + 1) * per) / grid * grid;
            sh[s].opt = &o; sh[s].shard = s;
            sh[s].first_frame = ((long long)s * per) / grid * grid;
            sh[s].frames = next - sh[s].first_frame;
            if (sh[s].frames <= 0) {
                fprintf(stderr, "--seamless-dc: %lld frames are too few for %d shards on a grid of %lld frames (lcm of 4096 and --chunk-frames): "
                                "shard %d would be empty\n", total_frames, o.shards, grid, s);
                return 1;
            }
            sh[s].preroll_frames = sh[s].first_frame < pre_calls ? sh[s].first_frame : pre_calls;
            uint64_t first_out = 0, nout = 0;
            if (iqgpu_design_out_frames_range(&o.desc, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) {
                fprintf(stderr, "%s\n", iqgpu_last_error()); return 1;
            }
            sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
            sh[s].planned_out = (long long)nout;
            if (o.dry && s < o.shards - 1) sh[s].n_dc_rows = (sh[s].frames + cf - 1) / cf;     /* rows pass 1 will record: one per call */
        }
        g_shards = sh;
        if (!o.dry && pthread_barrier_init(&g_pass, NULL, (unsigned)o.shards) != 0) { fprintf(stderr, "pthread_barrier_init failed\n"); return 1; }
    }
    if (o.seamless_dc_agc) {
        /* the preroll is the filters' memory alone -- the description with the blocker and the AGC off -- in whole calls; placement
         * depends on neither */
        iqgpu_chain_desc nd = o.desc;
        nd.dc_block_enable = 0; nd.agc_enable = 0;
        if (iqgpu_design_preroll_frames(&nd, &preroll) != IQGPU_OK) { fprintf(stderr, "--seamless-dc-agc: %s\n", iqgpu_last_error()); return 1; }
        const long long cf = (long long)o.chunk_frames, agc_chunk = o.desc.agc_chunk_frames ? (long long)o.desc.agc_chunk_frames : 16384;
        const long long pre_calls = ((long long)preroll + cf - 1) / cf * cf;
        long long grid = 4096;
        { long long x = grid, y = cf; while (y) { const long long t = x % y; x = y; y = t; } grid = grid / x * cf; }
        for (int s = 0; s < o.shards; s++) {
            const long long next = (s == o.shards - 1) ? total_frames : ((long long)(s + 1) * per) / grid * grid;
            sh[s].opt = &o; sh[s].shard = s;
            sh[s].first_frame = ((long long)s * per) / grid * grid;
            sh[s].frames = next - sh[s].first_frame;
            if (sh[s].frames <= 0) {
                fprintf(stderr, "--seamless-dc-agc: %lld frames are too few for %d shards on a grid of %lld frames (lcm of 4096 and --chunk-frames): "
                                "shard %d would be empty\n", total_frames, o.shards, grid, s);
                return 1;
            }
            sh[s].preroll_frames = sh[s].first_frame < pre_calls ? sh[s].first_frame : pre_calls;
            uint64_t first_out = 0, nout = 0;
            if (iqgpu_design_out_frames_range(&nd, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) {
                fprintf(stderr, "%s\n", iqgpu_last_error()); return 1;
            }
            sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
            sh[s].planned_out = (long long)nout;
            if (o.dry && s < o.shards - 1) {        /* what the measuring steps will record at least: one DC row per call (two for a cut one), one AGC row per chunk */
                sh[s].n_dc_rows = (sh[s].frames + cf - 1) / cf;
                sh[s].agc_rows = (sh[s].frames + agc_chunk - 1) / agc_chunk;
            }
        }
        g_shards = sh;
        if (!o.dry && pthread_barrier_init(&g_pass, NULL, (unsigned)o.shards) != 0) { fprintf(stderr, "pthread_barrier_init failed\n"); return 1; }
    }
    for (int s = 0; s < o.shards && !o.seamless && !o.seamless_agc && !o.seamless_dc && !o.seamless_dc_agc && !o.seamless_rms; s++) {
        sh[s].opt = &o; sh[s].shard = s;
        sh[s].first_frame = (long long)s * per;
        sh[s].frames = (s == o.shards - 1) ? total_frames - sh[s].first_frame : per;
        sh[s].out_offset_bytes = off;
        /* frames a fresh chain will produce for sh[s].frames input frames: the library's own closed form (decimating
         * or interpolating resampler, FFT-block quantisation in front of or behind it) */
        size_t nout = 0;
        if (iqgpu_design_out_frames(&o.desc, (size_t)sh[s].frames, &nout) != IQGPU_OK) { fprintf(stderr, "%s\n", iqgpu_last_error()); return 1; }
        sh[s].planned_out = (long long)nout;
        off += (long long)nout * (long long)obps;
    }
    if (o.out_path && !o.dry) { int fd = open(o.out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644); if (fd >= 0) close(fd); }

    const double t0 = now_s();
    pthread_t *th = (pthread_t *)calloc((size_t)o.shards, sizeof(pthread_t));
    for (int s = 0; s < o.shards; s++) pthread_create(&th[s], NULL, run_shard, &sh[s]);
    int rc = 0;
    long long frames_out = 0;
    double stream_s = 0;
    for (int s = 0; s < o.shards; s++) {
        pthread_join(th[s], NULL);
        if (sh[s].rc) { fprintf(stderr, "shard %d failed: %s\n", s, sh[s].err); rc = 1; }
        frames_out += sh[s].frames_out;
        if (sh[s].stream_seconds > stream_s) stream_s = sh[s].stream_seconds;
    }
    /* --seamless-rms: the seam certificate (iqgpu.h), in order.  Shard s started from the state shard s-1 ended in, bit for bit: its
     * bytes are the single stream's, given that shard s-1's are.  Otherwise its range again from shard s-1's checkpoint, in a thread
     * of its own like the first time, and the seam behind it is checked against the new end state. */
    int seams_certified = 0, ranges_redone = 0;
    for (int s = 1; s < o.shards && o.seamless_rms && !o.dry && rc == 0; s++) {
        const iqgpu_agc_state *e = &sh[s - 1].rms_end_state, *b = &sh[s].rms_seek_state;
        if (!memcmp(&e->current_gain, &b->current_gain, sizeof(float)) && !memcmp(&e->peak_memory, &b->peak_memory, sizeof(float)) &&
            e->samples_seen == b->samples_seen) { sh[s].certified = 1; seams_certified++; continue; }
        sh[s].redo_blob = sh[s - 1].blob; sh[s].redo_bytes = sh[s - 1].blob_bytes; sh[s].redone = 1; ranges_redone++;
        frames_out -= sh[s].frames_out;
        sh[s].rc = 0; sh[s].err[0] = 0;
        pthread_create(&th[s], NULL, run_shard, &sh[s]);
        pthread_join(th[s], NULL);
        if (sh[s].rc) { fprintf(stderr, "shard %d failed when its range was redone: %s\n", s, sh[s].err); rc = 1; }
        frames_out += sh[s].frames_out;
    }
    char mode_kv[160] = "";
    snprintf(mode_kv, sizeof(mode_kv), "%s", o.seamless ? "\"seamless\": true, " : o.seamless_agc ? "\"seamless_agc\": true, " : o.seamless_dc ? "\"seamless_dc\": true, " :
             o.seamless_dc_agc ? "\"seamless_dc_agc\": true, " : "");
    if (o.seamless_rms && o.dry) snprintf(mode_kv, sizeof(mode_kv), "\"seamless_rms\": true, ");
    else if (o.seamless_rms) snprintf(mode_kv, sizeof(mode_kv), "\"seamless_rms\": true, \"seams\": %d, \"seams_certified\": %d, \"ranges_redone\": %d, ", o.shards - 1,
                                      seams_certified, ranges_redone);
    const double dt = now_s() - t0;
    if (o.dry) {
        /* one JSON line: the placement as planned; `distinct_devices` is what an N-shard job on N GPUs must show */
        int distinct = 0;
        for (int s = 0; s < o.shards; s++) { int seen = 0; for (int q = 0; q < s; q++) if (!strcmp(sh[q].bus_id, sh[s].bus_id) && sh[q].device == sh[s].device) seen = 1; if (!seen) distinct++; }
        printf("{\"dry_placement\": true, %s\"frames_in\": %lld, \"frames_out\": %lld, \"shards\": %d, \"devices\": %d, \"distinct_devices\": %d, \"per_shard\": [",
               mode_kv, total_frames, frames_out, o.shards, o.devices, distinct);
        for (int s = 0; s < o.shards; s++) {
            char pre_kv[160] = "";
            if (o.seamless || o.seamless_rms) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld", sh[s].preroll_frames);
            if (o.seamless_agc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"agc_rows\": %lld", sh[s].preroll_frames, sh[s].agc_rows);
            if (o.seamless_dc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"dc_rows\": %lld", sh[s].preroll_frames, sh[s].n_dc_rows);
            if (o.seamless_dc_agc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"dc_rows\": %lld, \"agc_rows\": %lld", sh[s].preroll_frames, sh[s].n_dc_rows, sh[s].agc_rows);
            printf("%s{\"shard\": %d, \"device\": %d, \"pci_bus_id\": \"%s\", \"numa_node\": %d, \"cpus_allowed\": %d, \"first_frame\": %lld, \"frames_in\": %lld, \"planned_out\": %lld, "
                   "\"out_offset_bytes\": %lld, \"pinned_bytes\": %lld, \"hbm_bytes\": %lld%s}", s ? ", " : "", s, sh[s].device, sh[s].bus_id, sh[s].numa_node, sh[s].cpus_allowed,
                   sh[s].first_frame, sh[s].frames, sh[s].planned_out, sh[s].out_offset_bytes, sh[s].pinned_bytes, sh[s].hbm_bytes, pre_kv);
        }
        printf("]}\n");
        free(th); free(sh);
        return rc;
    }
    if (!o.quiet) {
        printf("{%s\"frames_in\": %lld, \"frames_out\": %lld, \"shards\": %d, \"devices\": %d, \"seconds\": %.6f, \"msps_end_to_end\": %.3f, \"stream_seconds\": %.6f, \"msps_streaming\": %.3f, "
               "\"h2d_GBs\": %.3f, \"d2h_GBs\": %.3f, \"in_bytes_per_frame\": %zu, \"out_bytes_per_frame\": %zu, \"input\": \"%s\", \"per_shard\": [",
               mode_kv, total_frames, frames_out, o.shards, o.devices, dt, total_frames / dt / 1e6, stream_s, stream_s > 0 ? total_frames / stream_s / 1e6 : 0.0,
               stream_s > 0 ? (double)total_frames * (double)ibps / stream_s / 1e9 : 0.0, stream_s > 0 ? (double)frames_out * (double)obps / stream_s / 1e9 : 0.0, ibps, obps,
               o.synthetic_frames <= 0 ? "file" : o.have_hash ? "synthetic-hash" : "synthetic-constant");
        for (int s = 0; s < o.shards; s++) {
            char pre_kv[512] = "";
            if (o.seamless) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld", sh[s].preroll_frames);
            if (o.seamless_rms) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"certified\": %s, \"redone\": %s, \"end\": {\"peak_memory\": %.9g, "
                "\"current_gain\": %.9g, \"samples_seen\": %llu}", sh[s].preroll_frames, sh[s].certified ? "true" : "false", sh[s].redone ? "true" : "false",
                (double)sh[s].rms_end_state.peak_memory, (double)sh[s].rms_end_state.current_gain, (unsigned long long)sh[s].rms_end_state.samples_seen);
            if (o.seamless_agc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"measure_seconds\": %.6f, \"agc_rows\": %lld, \"entry\": {\"locked\": %d, "
                "\"peak_memory\": %.9g, \"current_gain\": %.9g, \"last_strong_peak_time\": %.17g, \"samples_seen\": %llu}", sh[s].preroll_frames, sh[s].measure_seconds,
                sh[s].agc_rows, sh[s].entry.locked, (double)sh[s].entry.peak_memory, (double)sh[s].entry.current_gain, sh[s].entry.last_strong_peak_time,
                (unsigned long long)sh[s].entry.samples_seen);
            if (o.seamless_dc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"measure_seconds\": %.6f, \"dc_rows\": %lld, \"entry\": {\"re\": %.17g, \"im\": %.17g}",
                sh[s].preroll_frames, sh[s].measure_seconds, sh[s].n_dc_rows, sh[s].dc_entry.re, sh[s].dc_entry.im);
            if (o.seamless_dc_agc) snprintf(pre_kv, sizeof(pre_kv), ", \"preroll_frames\": %lld, \"measure_seconds\": %.6f, \"dc_rows\": %lld, \"agc_rows\": %lld, "
                "\"dc_entry\": {\"re\": %.17g, \"im\": %.17g}, \"entry\": {\"locked\": %d, \"current_gain\": %.9g, \"samples_seen\": %llu}", sh[s].preroll_frames,
                sh[s].measure_seconds, sh[s].n_dc_rows, sh[s].agc_rows, sh[s].dc_entry.re, sh[s].dc_entry.im, sh[s].entry.locked, (double)sh[s].entry.current_gain,
                (unsigned long long)sh[s].entry.samples_seen);
            printf("%s{\"shard\": %d, \"device\": %d, \"numa_node\": %d, \"first_frame\": %lld, \"frames_in\": %lld, \"frames_out\": %lld, \"planned_out\": %lld, \"out_offset_bytes\": %lld, \"seconds\": %.6f%s}",
                   s ? ", " : "", s, sh[s].device, sh[s].numa_node, sh[s].first_frame, sh[s].frames, sh[s].frames_out, sh[s].planned_out, sh[s].out_offset_bytes, sh[s].stream_seconds, pre_kv);
        }
        printf("]}\n");
    }
    for (int s = 0; s < o.shards; s++) if (sh[s].rows) iqgpu_host_free_pinned(sh[s].rows);
    for (int s = 0; s < o.shards; s++) { free(sh[s].dc_rows); free(sh[s].dc_call_rows); free(sh[s].blob); }
    free(th); free(sh);
    return rc;
}
