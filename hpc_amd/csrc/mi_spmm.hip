// mi_spmm.hip -- C ABI (include/mi_spmm.h) over the gfx950 kernels.
//
// Host side of the drop-in: what SpMMOpt::preprocess / SpMMOpt::run do in the
// reference (PA4/workspace/src/spmm_opt.cu:37-75), re-designed for MI355X:
//   preprocess: validate the CSR, detect block groups, classify rows and build the
//               segment table on the device (preprocess_gpu.hip; the reference-style
//               host loop stays behind gpu_preprocess=0), allocate the partial-sum
//               workspace (handle-owned);
//   run:        rows kernel (+ segments + reduce + blocks where such rows exist) on
//               the caller's stream; overwrite semantics; no host sync.
#include "../../include/mi_spmm.h"
#include "plan.hpp"
#include "spmm_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace mi;

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// The seven settings "autotune" may choose (0 = auto everywhere but fused_step, whose auto is 2).  The handle holds two copies: `user`, what set_option
// wrote, and `in_force`, what the plan and run_part use -- the caller's values, with the tuner's candidate or winner where the caller left one at auto.
struct Tunables {
    int64_t hub_thr;      // "long_row_threshold": rows longer than this are hubs (the resolved value in force: mi_spmm_handle::long_thr)
    int64_t medium_thr;   // "medium_row_threshold": rows longer than this (and not hubs) run as one exact segment in the segment kernel
    int64_t col_strips;   // "col_strips": column strips of the exact segments (plan.hpp): 1 = off, S >= 2 = that many (if the segments' columns ascend)
    int64_t tile_cols;    // "tile_cols": widest column tile of the rows/segment kernels: 256 (whole wave on a row), 128, 64, 32
    int64_t fused_step;   // "fused_step": 2 = auto, 0 = never, 1 = whenever the step is eligible: hub rows, segments and short rows as the three
                          // roles of ONE launch (spmm_kernels.hpp spmm_small_step) instead of 2-3 launches and a side-stream fork / join
    int64_t seg_order;    // "segment_order": 1 = segments longest first, 2 = in row order
    int64_t rows_unroll;  // "rows_unroll": B-row gathers in flight per lane group in the rows kernel: 8, 16
};

// "autotune_mask" (mi_spmm.h): bit 0 tile, 1 strips, 2 medium, 3 fused, 4 segment order, 5 rows unroll, 6 hub threshold -- the settings the tuner changed
static uint32_t tuned_settings(const Tunables &user, const Tunables &f)
{
    return (f.tile_cols != user.tile_cols ? 1u : 0u) | (f.col_strips != user.col_strips ? 2u : 0u) | (f.medium_thr != user.medium_thr ? 4u : 0u) |
           (f.fused_step != user.fused_step ? 8u : 0u) | (f.seg_order != user.seg_order ? 16u : 0u) | (f.rows_unroll != user.rows_unroll ? 32u : 0u) |
           (f.hub_thr != user.hub_thr ? 64u : 0u);
}

struct mi_spmm_handle {
    uint32_t magic;
    const int32_t *d_ptr;
    const int32_t *d_idx;
    const float *d_val;
    int32_t num_v, num_cols, feat;
    int64_t nnz;
    // options
    Tunables user, in_force;
    int64_t medium_res;  // the medium threshold in force after preprocess (auto resolved, capped by long_thr)
    int64_t split_long;   // 0 (default): hubs keep their stored order (spmm_hub); 1: hubs are cut into pieces summed piece by piece
    int64_t hub_slice;    // columns per hub wave: 16, 32, 64; 0 = auto
    int64_t hub_overlap;  // 1 (default): the hub kernel and the segment kernel run on handle-owned side streams, forked from and joined
                          // back into the caller's stream inside every run call (their longest rows then overlap the rows kernel)
    hipStream_t side[2];  // [0]: hub kernel, [1]: segment (+ reduce) kernels; created by the first preprocess that needs them
    int32_t side_overlaps[2]; // concurrent_stream's verdict on each side stream (1: its kernels run beside the null stream's)
    int64_t side_priority; // bit 0: the hub stream is a high-priority stream, bit 1: the segment stream is
    int64_t ftz;          // "flush_denormals": fp32 subnormals flushed like the reference's nvcc --use_fast_math build (spmm_kernels.hpp apply_ftz)
    int64_t segment_overlap; // 1: the segment kernel may go to side stream 1; 0: it stays on the caller's stream, in front of the rows kernel
    hipEvent_t ev_fork, ev_join[2];
    bool fork_recorded, forked[2];   // state of the current run_rows call
    bool overlap_on[2];   // resolved by preprocess: is the fork/join (~20 us of launch latency per call) worth it for this class
    int64_t long_thr;     // the hub threshold in force (resolved by preprocess; before it, the caller's value)
    int64_t long_chunk, rows_per_block, xcd_remap, nt_store, nt_stream, block_path;
    int64_t block_threads;  // v2 workgroup size: 64, 128 or 256
    int64_t gpu_preprocess;  // 1: segment table built on the device (default); 0: reference-style host loop
    int64_t kernel;  // 2 = spmm_rows_v2 (pipelined items); 1 named the first-generation kernel, retired in round 3
    int64_t split_cols;  // 1 (default): columns past the last full 256-column tile get their own launches
    int64_t segment_unroll;  // B-row gathers in flight per lane group in the segment kernel: 8, 16 or 32 (default)
    Chunk *d_strips;         // [n_strips][n_chunks] sub-segments, strip-major; grow-only buffer (capacity strips_cap sub-segments), kept across preprocess calls
    size_t strips_cap;
    int32_t n_strips;        // strips in force (1 = none)
    int32_t seg_unsorted;    // segments whose columns do not ascend (-1: not looked at)
    int64_t seg_nnz;         // nonzeros in the whole segments (either plan builder): the strip rule's input, known before any column is read
    int64_t strips_builder;  // 0 (default): strip_segments, one pass; 1: the round-4 pair survey_segments + build_col_strips (cross-check)
    int32_t last_fused;      // 1: the last run call went through the small-step kernel
    int64_t fused_order;     // "fused_order": 0 (default) = auto, 1 = hub workgroups first in the small-step grid, 2 = segment workgroups first
    int32_t last_seg_first;  // 1: the last small-step launch put its segment workgroups first
    int32_t last_rows_deep;  // 1: the last rows launch kept 16 gathers in flight per lane group
    // "autotune" (round 5): the rules above are guesses from a 8 192-row sample and a histogram; a wrong guess is silent (same bits, slower).  With the option on,
    // preprocess MEASURES: the step is timed on the buffers it is given (the reference's preprocess touches vout too: spmm_opt.cu:67) under the auto plan and
    // under a handful of forced settings of the options the caller left to us -- tile width, strip count, medium threshold, one launch or several -- and the
    // fastest is kept (in_force; user is never touched).  Scheduling only: whatever wins gives the same bits.
    int64_t autotune;
    int32_t tune_evals;      // candidate settings timed by the last preprocess
    double tune_auto_ms, tune_best_ms;
    // plan
    bool prepared;
    Chunk *d_chunks;
    LongRow *d_long;
    float *d_partials;
    int32_t n_chunks, n_long, n_medium, n_slots;
    int64_t ldp;
    size_t ws_bytes;
    int32_t max_row_nnz;
    int32_t local_pct;   // column locality sample (percent); -1 = not measured
    int32_t front_pct;   // sampled nonzeros in the first quarter of the columns (percent; uniform columns: 25)
    double preprocess_us;
    double phase_us[5];  // set-up, column check, block detection, plan tables (either builder, strips, rebuild), partial sums + block items
    int32_t last_lpr, last_v, last_launches, last_wide;
    // block (MFMA) path
    int64_t block_min_len;
    uint8_t *d_blk_flag;
    int32_t *d_blk_groups;
    int32_t n_blk_groups;
    int64_t n_rows_for_rows_kernel;  // rows neither split nor owned by the block path
    // block path, run time: pieces of the groups' column lists, grouped into items, per pass (spmm_kernels.hpp)
    int64_t block_share;       // most pieces per item (1 = no sharing; default 2)
    int64_t block_max_pieces;  // most pieces a group's list is cut into = most passes (1 = never cut)
    int64_t block_wg_waves;    // waves (= items) per workgroup of the block kernels: 1 (default), 2, 4
    int64_t block_run_min;     // shortest run worth a piece of its own
    BlockItem *d_blk_items;    // grow-only (capacity blk_items_cap items): kept across preprocess calls, released by destroy
    size_t blk_items_cap;
    int32_t n_blk_items, n_blk_pieces, n_blk_passes, n_blk_shared_items;
    // preprocess temporaries (grow-only, kept across preprocess calls, released by destroy)
    Scratch scratch_a, scratch_b;
    unsigned int *d_col_bad;   // 256 bytes: the column-range flag
    struct { int32_t off, n; } blk_launch[kMaxPieces][3];   // [pass][0: list items, 1: run items of one piece, 2: shared run items]
    std::vector<int32_t> *hub_rows_sorted;   // host copy of the hub rows, ascending (null: unknown -> every call launches the hub kernel)
};

static const uint32_t kMagic = 0x4d49534du;  // "MISM"
// Pieces of a split row: the plan builders step through a row in int32; a piece length far beyond any row
// that can be split usefully would overflow `b + clen`.
static const int64_t kMaxLongChunk = 1 << 20;

static bool good(const mi_spmm_handle *h) { return h && h->magic == kMagic; }

static void free_plan(mi_spmm_handle *h)
{
    if (h->d_chunks) (void)hipFree(h->d_chunks);
    h->n_strips = 1;         // (the strip buffer itself is grow-only: released by destroy)
    h->seg_unsorted = -1;
    h->seg_nnz = 0;
    if (h->d_long) (void)hipFree(h->d_long);
    if (h->d_partials) (void)hipFree(h->d_partials);
    if (h->d_blk_flag) (void)hipFree(h->d_blk_flag);
    if (h->d_blk_groups) (void)hipFree(h->d_blk_groups);
    h->n_blk_items = h->n_blk_pieces = h->n_blk_passes = h->n_blk_shared_items = 0;
    std::memset(h->blk_launch, 0, sizeof(h->blk_launch));
    h->d_blk_flag = nullptr;
    h->d_blk_groups = nullptr;
    h->n_blk_groups = 0;
    h->d_chunks = nullptr;
    h->d_long = nullptr;
    h->d_partials = nullptr;
    h->n_chunks = h->n_long = h->n_medium = h->n_slots = 0;
    delete h->hub_rows_sorted;
    h->hub_rows_sorted = nullptr;
    h->local_pct = -1;
    h->front_pct = 25;
    h->ws_bytes = 0;
    h->prepared = false;
}

// The block kernel works on column slabs of 256/128/64/32 columns (blockIdx.y walks them): any N that is
// a multiple of 32 qualifies, with the widest slab that divides it.
static int block_slab_width(int32_t N) { return N <= 0 ? 0 : (N % 256 == 0 ? 256 : N % 128 == 0 ? 128 : N % 64 == 0 ? 64 : N % 32 == 0 ? 32 : 0); }
static bool block_path_shape_ok(int32_t N) { return block_slab_width(N) != 0; }

// Block path, second half of preprocess: the qualifying groups (d_blk_groups, either plan builder) are cut into
// pieces on the device (analyze_group_runs: one wave per group, O(nnz / 16) reads); every pass's pieces are ordered by
// first column and formed into items: run pieces with the same first column share their B rows (longest first, at most
// block_share per item, every shared length a whole number of k batches so that no shared piece ends inside a batch).
// On the device by default (preprocess_gpu.hip build_block_items_gpu: one radix sort, two scans, one 80-byte copy back);
// the host assembler below -- the pieces come back, O(groups log groups) on one core: 8 ms for C4's 65 536 groups --
// stays behind "gpu_preprocess" = 0 as the cross-check (test_gpu_and_host_plan_builders_agree: same items, same launches).
static int build_block_items(mi_spmm_handle *h)
{
    const int32_t ng = h->n_blk_groups;
    if (ng <= 0) return MI_SPMM_OK;
    // the groups' pieces live in the first preprocess arena (build_plan_gpu is done with it): no allocation call here
    if (scratch_reserve(&h->scratch_a, (size_t)ng * sizeof(GroupPieces) + 256) != 0) return MI_SPMM_ENOMEM;
    GroupPieces *d_gp = reinterpret_cast<GroupPieces *>(h->scratch_a.p);
    hipLaunchKernelGGL(analyze_group_runs, dim3((unsigned)((ng + 3) / 4)), dim3(kBlockThreads), 0, 0, h->d_ptr, h->d_idx,
                       h->d_blk_groups, ng, (int32_t)h->block_max_pieces, (int32_t)h->block_run_min, d_gp);
    hipError_t e = hipGetLastError();
    // shared items need the two-piece kernels, which exist for 256- and 128-column slabs (N % 128 == 0)
    const int slab_w = block_slab_width(h->feat);
    const int share = slab_w >= 128 ? (int)h->block_share : 1;
    // the run kernels sweep whole trips (two k batches: 16 / 32 / 64 rows for 256- / 128- / narrower slabs) and fetch their A
    // operands 16 bytes at a time; a run of any other length goes through the list kernel (general lengths, dword A loads)
    const int run_unit = slab_w == 256 ? 16 : slab_w == 128 ? 32 : 64;
    if (e == hipSuccess && h->gpu_preprocess) {
        BlockPlanOut bo;
        bo.d_items = h->d_blk_items;
        bo.items_cap = h->blk_items_cap;
        const int rc = build_block_items_gpu(d_gp, h->d_blk_groups, ng, share, run_unit, &h->scratch_b, &bo);
        h->d_blk_items = bo.d_items;
        h->blk_items_cap = bo.items_cap;
        if (rc != MI_SPMM_OK) return rc;
        h->n_blk_items = bo.n_items;
        h->n_blk_pieces = bo.n_pieces;
        h->n_blk_passes = bo.n_passes;
        h->n_blk_shared_items = bo.n_shared;
        h->ws_bytes += (size_t)bo.n_items * sizeof(BlockItem);
        const int run_cls = share > 1 ? 2 : 1;     // run items of one and of two pieces share a launch where the two-piece kernels exist
        for (int pass = 0; pass < kMaxPieces; ++pass) {
            h->blk_launch[pass][0].off = bo.launch[pass][0].off;
            h->blk_launch[pass][0].n = bo.launch[pass][0].n;
            h->blk_launch[pass][run_cls].off = bo.launch[pass][1].off;
            h->blk_launch[pass][run_cls].n = bo.launch[pass][1].n;
        }
        return MI_SPMM_OK;
    }
    std::vector<GroupPieces> gp((size_t)ng);
    std::vector<int32_t> groups((size_t)ng);
    if (e == hipSuccess) e = hipMemcpy(gp.data(), d_gp, (size_t)ng * sizeof(GroupPieces), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(groups.data(), h->d_blk_groups, (size_t)ng * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;

    struct Key { int32_t col, len, gi, ord; bool shareable, run; };
    struct Launch { int32_t off, n; };
    std::vector<BlockItem> items;
    int64_t n_pieces = 0;
    int32_t n_pass = 0, n_shared = 0;
    std::vector<Key> keys;
    std::vector<BlockItem> lists, singles, shared;

    auto piece_of = [&](const Key &k) {
        const GroupPieces &g = gp[(size_t)k.gi];
        BlockPiece p;
        p.group = groups[(size_t)k.gi];
        p.k0 = g.k0[k.ord];
        p.len = g.len[k.ord];
        p.flags = (k.ord > 0 ? kPieceCarryIn : 0) | (k.ord + 1 < g.n ? kPieceCarryOut : 0);
        p.p0 = g.p0;
        p.row_len = g.row_len;
        return p;
    };
    // one pass's keys -> its items, appended to `out` class by class (lists, singles, shared)
    auto form_items = [&](std::vector<Key> &ks, std::vector<BlockItem> &out, Launch (&launch)[3], bool count) {
        // by first column; among equals the shareable ones together, longest first; ties in group order (deterministic)
        std::sort(ks.begin(), ks.end(), [](const Key &x, const Key &y) {
            if (x.col != y.col) return x.col < y.col;
            if (x.shareable != y.shareable) return x.shareable > y.shareable;
            if (x.len != y.len) return x.len > y.len;
            return x.gi < y.gi;
        });
        lists.clear();
        singles.clear();
        shared.clear();
        size_t i = 0;
        while (i < ks.size()) {
            size_t j = i + 1;
            if (ks[i].shareable)
                while (j < ks.size() && j - i < (size_t)share && ks[j].shareable && ks[j].col == ks[i].col) ++j;
            BlockItem it;
            std::memset(&it, 0, sizeof(it));
            it.m = (int32_t)(j - i);
            it.c0 = ks[i].run ? ks[i].col : -1 - ks[i].col;
            for (size_t q = i; q < j; ++q) it.p[q - i] = piece_of(ks[q]);
            // run items of one and of two pieces go through the same launch where the two-piece kernels exist: one long
            // list in column order instead of two short ones (a short launch pays its tail on 256 CUs)
            (it.c0 < 0 ? lists : (it.m > 1 || share > 1) ? shared : singles).push_back(it);
            if (count) {
                n_pieces += it.m;
                if (it.m > 1) ++n_shared;
            }
            i = j;
        }
        std::vector<BlockItem> *cls[3] = {&lists, &singles, &shared};
        for (int c = 0; c < 3; ++c) {
            launch[c].off = (int32_t)out.size();
            launch[c].n = (int32_t)cls[c]->size();
            out.insert(out.end(), cls[c]->begin(), cls[c]->end());
        }
    };
    for (int pass = 0; pass < kMaxPieces; ++pass) {
        keys.clear();
        for (int32_t gi = 0; gi < ng; ++gi) {
            const GroupPieces &g = gp[(size_t)gi];
            for (int ord = 0; ord < g.n; ++ord) {
                if (ord != pass) continue;
                Key k;
                const int32_t c = g.c0[ord];
                k.run = c >= 0 && g.len[ord] % run_unit == 0;      // any other run the run kernels cannot take: a list piece
                k.col = c >= 0 ? c : -1 - c;
                k.len = g.len[ord];
                k.gi = gi;
                k.ord = ord;
                k.shareable = k.run && (g.len[ord] % kShareLenUnit) == 0 && share > 1;
                keys.push_back(k);
            }
        }
        if (keys.empty()) break;
        n_pass = pass + 1;
        Launch al[3];
        form_items(keys, items, al, true);
        for (int c = 0; c < 3; ++c) { h->blk_launch[pass][c].off = al[c].off; h->blk_launch[pass][c].n = al[c].n; }
    }
    if (items.empty()) return MI_SPMM_OK;

    auto upload = [&](void **dst, const void *src, size_t bytes) -> int {
        if (bytes == 0) return MI_SPMM_OK;
        if (hipMalloc(dst, bytes) != hipSuccess) return MI_SPMM_ENOMEM;
        const hipError_t ue = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        if (ue != hipSuccess) return (int)ue;
        h->ws_bytes += bytes;
        return MI_SPMM_OK;
    };
    if (h->blk_items_cap < items.size()) {
        if (h->d_blk_items) (void)hipFree(h->d_blk_items);
        h->d_blk_items = nullptr;
        h->blk_items_cap = 0;
    }
    int rc = MI_SPMM_OK;
    if (h->d_blk_items) {
        const hipError_t ue = hipMemcpy(h->d_blk_items, items.data(), items.size() * sizeof(BlockItem), hipMemcpyHostToDevice);
        if (ue != hipSuccess) rc = (int)ue;
        else h->ws_bytes += items.size() * sizeof(BlockItem);
    } else {
        rc = upload((void **)&h->d_blk_items, items.data(), items.size() * sizeof(BlockItem));
        if (rc == MI_SPMM_OK) h->blk_items_cap = items.size();
    }
    if (rc != MI_SPMM_OK) return rc;
    h->n_blk_items = (int32_t)items.size();
    h->n_blk_pieces = (int32_t)n_pieces;
    h->n_blk_passes = n_pass;
    h->n_blk_shared_items = n_shared;
    return MI_SPMM_OK;
}

// Host copy of the hub rows in row order: a run_rows call (a row panel of the multi-GPU step) whose range holds no hub row
// skips the hub launch and its side-stream fork (~20 us) instead of launching a grid whose workgroups all leave at once.
static int note_hub_rows(mi_spmm_handle *h)
{
    delete h->hub_rows_sorted;
    h->hub_rows_sorted = nullptr;
    if (h->n_long <= 0 || h->split_long || h->n_long > (1 << 16)) return MI_SPMM_OK;
    std::vector<LongRow> lr((size_t)h->n_long);
    HIP_TRY(hipMemcpy(lr.data(), h->d_long, lr.size() * sizeof(LongRow), hipMemcpyDeviceToHost));
    h->hub_rows_sorted = new (std::nothrow) std::vector<int32_t>();
    if (!h->hub_rows_sorted) return MI_SPMM_ENOMEM;
    h->hub_rows_sorted->reserve(lr.size());
    for (const LongRow &r : lr) h->hub_rows_sorted->push_back(r.row);
    std::sort(h->hub_rows_sorted->begin(), h->hub_rows_sorted->end());
    return MI_SPMM_OK;
}

static bool range_has_hub(const mi_spmm_handle *h, int32_t row_begin, int32_t row_end)
{
    if (!h->hub_rows_sorted) return true;
    const auto it = std::lower_bound(h->hub_rows_sorted->begin(), h->hub_rows_sorted->end(), row_begin);
    return it != h->hub_rows_sorted->end() && *it < row_end;
}

// The hub kernel's longest row is the step's longest dependent chain; on a side stream it runs beside the rows kernel
// instead of in front of it.  The stream and its two events belong to the handle (created once, here, never in run()).
// A side stream is only worth its fork if its kernels RUN BESIDE the caller's.  The runtime hands a process's streams a few hardware
// queues per priority, in creation order, and the queues sit on a handful of command-processor pipes: a high-priority queue that shares its
// pipe with the caller's queue is served FIRST, not alongside -- the hub kernel then runs alone and the rows kernel after it (youtube-shaped
// N = 32: 0.32 ms instead of 0.17), and which handle gets such a queue is a matter of how many streams the process has made before
// (every other handle in a loop that makes one stream per handle: profiles/r04_side_streams.txt).  So a candidate stream is TESTED: a 40 us
// spin kernel on it and one on the null stream (the reference's stream, util.h:133-136, and torch's default) -- beside each other they take
// ~40 us, one after the other ~80 -- and a stream that fails is kept aside (so that the next one made gets another queue) until one passes
// or four have been tried.  preprocess only (it synchronises anyway); ~0.2 ms per candidate, once per handle.
static int concurrent_stream(hipStream_t *out, int priority, int *overlaps_out)
{
    constexpr int kTries = 4;
    hipStream_t cand[kTries] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t e0 = nullptr, e1 = nullptr, ef = nullptr, ej = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ef, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ej, hipEventDisableTiming);
    int chosen = -1, made = 0;
    const unsigned long long ticks = 4000;      // 40 us of the 100 MHz counter
    for (int t = 0; t < kTries && e == hipSuccess && chosen < 0; ++t) {
        e = hipStreamCreateWithPriority(&cand[t], hipStreamNonBlocking, priority);
        if (e != hipSuccess) break;
        ++made;
        float best = 1e30f;
        for (int rep = 0; rep < 2 && e == hipSuccess; ++rep) {      // the first pair also pays the queue's first use
            e = hipEventRecord(e0, nullptr);
            if (e == hipSuccess) e = hipEventRecord(ef, nullptr);
            if (e == hipSuccess) e = hipStreamWaitEvent(cand[t], ef, 0);
            if (e == hipSuccess) { hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, cand[t], ticks, (unsigned int *)nullptr); e = hipGetLastError(); }
            if (e == hipSuccess) { hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, nullptr, ticks, (unsigned int *)nullptr); e = hipGetLastError(); }
            if (e == hipSuccess) e = hipEventRecord(ej, cand[t]);
            if (e == hipSuccess) e = hipStreamWaitEvent(nullptr, ej, 0);
            if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        if (std::getenv("MI_SPMM_DEBUG")) std::fprintf(stderr, "[mi_spmm] side stream candidate %d: spin pair %.1f us\n", t, best * 1e3f);
        if (e == hipSuccess && best < 0.078f) chosen = t;          // measured: 65-70 us beside each other (40 + launch and event overhead), 88-120 one after the other
    }
    const int keep = chosen >= 0 ? chosen : 0;
    for (int t = 0; t < made; ++t)
        if (t != keep && cand[t]) (void)hipStreamDestroy(cand[t]);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ef) (void)hipEventDestroy(ef);
    if (ej) (void)hipEventDestroy(ej);
    if (e != hipSuccess) { if (made > 0 && cand[keep]) (void)hipStreamDestroy(cand[keep]); return (int)e; }
    *out = cand[keep];
    *overlaps_out = chosen >= 0 ? 1 : 0;
    return MI_SPMM_OK;
}

static int ensure_side_streams(mi_spmm_handle *h)
{
    // A fork + join costs ~20 us of launch latency per run call (ddi-shaped N = 32: 0.047 -> 0.069 ms): worth it once the
    // step is long enough to hide something behind (estimate >= 0.2 ms) or the longest hub alone is a 50 us chain.
    // "hub_overlap": 0 = never, 1 = this rule, 2 = always.
    constexpr double kFabricRate = 6e12;
    const bool long_step = gather_bytes(h->nnz, h->num_v, h->feat) / kFabricRate >= 200e-6;
    const bool exact_hubs = h->n_long > 0 && !h->split_long;
    h->overlap_on[0] = exact_hubs && (h->hub_overlap == 2 || (h->hub_overlap == 1 && (long_step || h->max_row_nnz >= 7000)));
    // The segment kernel gets a side stream of its own only where that was measured to pay (interleaved A/B over twelve graph shapes x three widths,
    // profiles/r04_side_streams.txt): narrow B (N <= 64: both the rows kernel, 8 lanes per row, and the segment chains are latency-bound and fill
    // each other's gaps -- citation- and wikikg2-shaped N = 32: -8 %) and no hub stream beside it.  Everywhere else a second stream is neutral to
    // harmful (+0 .. +16 %: protein-shaped N = 32, with 1 696 hubs on their stream): the segment kernel then stays on the caller's stream.
    // Round 5 (structured graphs, profiles/r05_regret.md): where the columns are local the rows kernel is fast (its neighbours share B rows in L2) and the
    // segment chains in front of it are what the step waits for -- beside it they cost nothing: segment_overlap = 1 is 0.78 - 0.94 of the time on
    // yelp- / products- / ppa- / youtube- / citation-community at every width; the round-4 A/B (uniformly random columns) found it neutral to harmful there.
    const bool seg_side = h->segment_overlap == 1 || (h->segment_overlap == 2 && ((!h->overlap_on[0] && h->feat <= 64) || h->local_pct >= 50));
    h->overlap_on[1] = seg_side && h->n_chunks > 0 && (h->hub_overlap == 2 || (h->hub_overlap == 1 && long_step));
    if (!(h->overlap_on[0] || h->overlap_on[1])) return MI_SPMM_OK;
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (!h->ev_fork) HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) {
        if (!h->overlap_on[i] || h->side[i]) continue;          // made once per handle, and only the ones this plan uses
        int ov = 0;
        const int rc = concurrent_stream(&h->side[i], ((h->side_priority >> i) & 1) ? hi : 0, &ov);
        if (rc != MI_SPMM_OK) return rc;
        h->side_overlaps[i] = ov;
        HIP_TRY(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
    }
    return MI_SPMM_OK;
}

// The stream kernel class i of this run_rows call goes to: side stream i, made to wait for what the caller's stream holds
// so far (one fork event per call), or the caller's stream itself when overlap is off.
static int side_stream(mi_spmm_handle *h, int i, hipStream_t s, hipStream_t *out)
{
    *out = s;
    if (!h->overlap_on[i] || !h->side[i]) return MI_SPMM_OK;
    if (!h->fork_recorded) {
        HIP_TRY(hipEventRecord(h->ev_fork, s));
        h->fork_recorded = true;
    }
    if (!h->forked[i]) {
        HIP_TRY(hipStreamWaitEvent(h->side[i], h->ev_fork, 0));
        h->forked[i] = true;
    }
    *out = h->side[i];
    return MI_SPMM_OK;
}

namespace { int resolve_tile_cols(const mi_spmm_handle *h, int32_t N); }

// Column strips of the exact segments (plan.hpp), after either plan builder: the rule's cheap gates first, then one pass over
// the segments' columns (ascending? how many nonzeros?), then the S sub-segment tables.
static int plan_col_strips(mi_spmm_handle *h)
{
    h->n_strips = 1;
    h->seg_unsorted = -1;
    const int64_t want = h->in_force.col_strips;
    if (want == 1 || h->n_chunks <= 0 || h->split_long || h->n_slots > 0 || h->feat <= 0 || h->num_cols < 2) return MI_SPMM_OK;
    // width of a column tile of the segment kernel at this handle's N (run_part: lane groups of N/4 lanes, capped by the tile rule)
    const int V = h->feat >= 4 ? 4 : 1;
    int lpr = 1;
    while (lpr < (h->feat + V - 1) / V) lpr <<= 1;
    lpr = lpr < 8 ? 8 : (lpr > 64 ? 64 : lpr);
    const int cap = resolve_tile_cols(h, h->feat) / V;
    if (V == 4 && lpr > cap) lpr = cap;
    int tile = lpr * V;
    if (tile > h->feat) tile = h->feat;
    // (Round 4 left graphs with >= 50 % of their nonzeros near the diagonal alone: "neighbouring rows share their B rows through L2 already".  They do not
    //  once the rows are long: protein- / reddit-community (58 - 60 % local) 0.57 - 0.67 of the time with strips, and a BANDED matrix of 300-700-nonzero rows
    //  (100 % local: a row sits inside one or two strips) 0.54 - 0.69 -- the segment table is sorted by length, so a launch's rows come from all over the band.
    //  The gate is gone: profiles/r05_regret.md.)
    if (want == 0 && h->local_pct >= 95) return MI_SPMM_OK;      // banded / mesh: the rows stay in the rows kernel (medium rule), nothing long is left to strip
    if (want == 0 && resolve_col_strips(h->num_cols, tile, h->nnz, h->n_chunks, h->nnz, h->front_pct, h->local_pct) < 2) return MI_SPMM_OK;   // cannot pay whatever the survey says
    if (!h->d_col_bad) HIP_TRY(hipMalloc((void **)&h->d_col_bad, 256));
    void *d_sv = (char *)h->d_col_bad + 64;            // (the first bytes hold the column-range flag a second plan reads again)
    SegmentSurvey sv;
    if (h->strips_builder == 1) {                      // round 4: survey first (its nonzero count feeds the rule), tables afterwards
        const int rc = survey_segments(h->d_chunks, h->n_chunks, h->d_idx, d_sv, &sv);
        if (rc != 0) return rc;
        h->seg_unsorted = (int32_t)sv.unsorted;
        if (sv.unsorted) return MI_SPMM_OK;            // a row whose columns do not ascend cannot be cut by column without changing its order
        if ((int64_t)sv.nnz != h->seg_nnz) return MI_SPMM_ESTATE;      // the plan builders' count and the survey's are the same number
    }
    int64_t S = want >= 2 ? want : resolve_col_strips(h->num_cols, tile, h->seg_nnz, h->n_chunks, h->nnz, h->front_pct, h->local_pct);
    // local columns at a narrow B: a long row's nonzeros cluster in one or two strips, the other launches find it empty -- many strips only add launches
    // (ppa-community kLen 32: 14 strips DOUBLED the step, 4 are neutral, 2 take a fifth off; reddit- / protein-community kLen 32: 2 - 4 strips 0.88 - 0.95 of the time, 6 the same as none)
    if (want == 0 && h->local_pct >= 50 && h->feat < 128 && S > 2) S = 2;
    // a strip is a launch: ~10 us of ramp each.  Not more strips than the step has 0.1 ms slices of work (hold-out: an R-MAT of scale 18 at kLen 32 -- 0.17 ms
    // of bytes -- lost 30 % to six strips; every fitted case has >= 0.14 ms per strip)
    if (want == 0) {
        constexpr double kFabricRate = 6e12;
        const double step = gather_bytes(h->nnz, h->num_v, h->feat) / kFabricRate;
        const int64_t by_time = (int64_t)(step / 100e-6);
        if (S > by_time) S = by_time;
    }
    if (S > h->num_cols) S = h->num_cols;
    if (S > kMaxColStrips) S = kMaxColStrips;
    if (S < 2) return MI_SPMM_OK;
    const size_t need = (size_t)S * (size_t)h->n_chunks, bytes = need * sizeof(Chunk);
    if (h->strips_cap < need) {
        if (h->d_strips) (void)hipFree(h->d_strips);
        h->d_strips = nullptr;
        h->strips_cap = 0;
        if (hipMalloc((void **)&h->d_strips, bytes) != hipSuccess) { h->d_strips = nullptr; return MI_SPMM_ENOMEM; }
        h->strips_cap = need;
    }
    if (h->strips_builder == 1) {
        const int brc = build_col_strips(h->d_chunks, h->n_chunks, h->d_idx, h->num_cols, (int32_t)S, h->d_strips);
        if (brc != 0) return brc;
    } else {                                           // one pass: ascending? and the tables, which an unsorted segment leaves unusable
        const int brc = strip_segments(h->d_chunks, h->n_chunks, h->d_idx, h->num_cols, (int32_t)S, h->d_strips, d_sv, &sv);
        if (brc != 0) return brc;
        h->seg_unsorted = (int32_t)sv.unsorted;
        if (sv.unsorted) return MI_SPMM_OK;
    }
    h->n_strips = (int32_t)S;
    h->ws_bytes += bytes;
    return MI_SPMM_OK;
}

// The hub threshold a plan builder is given, from a setting: the caller's "long_row_threshold", a tuner's candidate, or the fold's 1 << 30.  Rows up to
// it stay ONE exact segment of the segment kernel; longer ones (hubs) go to the hub kernel (stored order) or, with "split_long_rows", are cut into pieces.
//   an explicit value is taken as is;
//   auto, split mode: 2048 once there is enough work to hide a 2048-nonzero segment (nnz >= 2^24), proportionally lower for small matrices
//     (profiles/r01_thresholds.txt);
//   auto, exact mode: 0 -- the builder resolves it from the row-length histogram (plan.hpp resolve_hub_threshold).
// The hub kernel moves 16-byte parts of B rows: in exact mode a B narrower than one part keeps its long rows as single exact segments of the segment
// kernel, whatever the setting (slow on a real hub, but N < 4 has no bandwidth to speak of either way).
static int64_t hub_threshold_for(const mi_spmm_handle *h, int64_t setting)
{
    if (!h->split_long && h->feat < 4) return INT32_MAX;
    if (setting > 0) return setting;
    if (!h->split_long) return 0;
    const int64_t t = h->nnz / 8192;
    return t < 256 ? 256 : (t > 2048 ? 2048 : t);
}

// The reference-style host loop ("gpu_preprocess" = 0), kept as the cross-check of build_plan_gpu (preprocess_gpu.hip): the same PlanOut from row_ptr
// copied back -- validation, histogram, column sample, the two threshold rules, classification, sort, upload.  The segment table is the reference's Task
// list (spmm_opt.cu:43-54), kept only for rows that need it:
//   len > thr                 -> hub: listed (exact mode) or cut into pieces of clen nonzeros, partial sums + ordered reduce (split mode)
//   mthr < len <= thr         -> ONE segment = the whole row, stored straight to C (exact order)
// Rows of block-path groups are excluded.  Segments are sorted longest first: neighbours in a wave have similar lengths and the tail is short.
static int build_plan_host(const int32_t *d_row_ptr, const int32_t *d_col_idx, int32_t M, int32_t K, int32_t N, int64_t nnz,
                           const uint8_t *d_blk_flag, const unsigned int *d_col_bad, int32_t mthr_user, int32_t thr_user, int32_t clen, int32_t split,
                           int32_t seg_order, void *d_scratch256, PlanOut *out)
{
    *out = PlanOut();
    std::vector<int32_t> ptr((size_t)M + 1);
    HIP_TRY(hipMemcpy(ptr.data(), d_row_ptr, sizeof(int32_t) * ((size_t)M + 1), hipMemcpyDeviceToHost));
    unsigned int col_bad = 0;
    if (d_col_bad) HIP_TRY(hipMemcpy(&col_bad, d_col_bad, sizeof(col_bad), hipMemcpyDeviceToHost));
    // data.cu:40-45 asserts ptr[num_v] == num_e; monotone rows and in-range columns keep the kernels in bounds
    if (col_bad || ptr[0] < 0 || (int64_t)ptr[M] != nnz) return MI_SPMM_ECSR;
    LenHist hist;
    std::memset(&hist, 0, sizeof(hist));
    int32_t max_len = 0;
    for (int32_t r = 0; r < M; ++r) {
        const int32_t len = ptr[r + 1] - ptr[r];
        if (len < 0) return MI_SPMM_ECSR;
        if (len > max_len) max_len = len;
        for (int i = 0; i < kHistN && len > hist_threshold(i); ++i) { ++hist.cnt[i]; hist.nnz[i] += (unsigned long long)len; }
    }
    const int src = sample_columns_gpu(d_row_ptr, d_col_idx, M, K, nnz, d_scratch256, &out->local_pct, &out->front_pct);
    if (src != 0) return src;
    const int32_t thr = thr_user > 0 ? thr_user : resolve_hub_threshold(nnz, M, K, N, hist.nnz, max_len);
    const int32_t mthr = resolve_medium_threshold(mthr_user, nnz, M, max_len, thr, out->local_pct, N);
    out->max_len = max_len;
    out->thr = thr;
    out->mthr = mthr;
    std::vector<uint8_t> flags;
    if (d_blk_flag) {
        flags.resize((size_t)(M + 15) / 16);
        HIP_TRY(hipMemcpy(flags.data(), d_blk_flag, flags.size(), hipMemcpyDeviceToHost));
        std::vector<int32_t> groups;
        for (size_t g = 0; g < flags.size(); ++g) if (flags[g]) groups.push_back((int32_t)g);
        if (!groups.empty()) {
            if (hipMalloc((void **)&out->d_blk_groups, groups.size() * sizeof(int32_t)) != hipSuccess) return MI_SPMM_ENOMEM;
            HIP_TRY(hipMemcpy(out->d_blk_groups, groups.data(), groups.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            out->n_blk_groups = (int32_t)groups.size();
        }
    }
    std::vector<Chunk> chunks;
    std::vector<LongRow> longs;
    for (int32_t r = 0; r < M && max_len > mthr; ++r) {
        const int32_t beg = ptr[r], end = ptr[r + 1], len = end - beg;
        if (len <= mthr) continue;
        if (out->n_blk_groups > 0 && flags[(size_t)(r >> 4)]) continue;      // block path owns it, whatever its length
        if (len <= thr) {
            chunks.push_back(Chunk{beg, end, -1, r});
            ++out->n_medium;
            out->seg_nnz += len;
            continue;
        }
        LongRow L{r, -1, 0, len};         // exact order: the hub kernel walks the row whole
        if (split) {
            L.first_slot = out->n_slots;
            for (int32_t b = beg; b < end; b += (end - b > clen ? clen : end - b)) {
                chunks.push_back(Chunk{b, (end - b > clen) ? b + clen : end, out->n_slots++, r});
                ++L.n_chunks;
            }
        }
        longs.push_back(L);
    }
    // hub rows longest first, ties in row order (as the device builder's stable radix sort leaves them)
    std::stable_sort(longs.begin(), longs.end(), [](const LongRow &x, const LongRow &y) { return x.len > y.len; });
    // segments longest first, stable -- unless the row order was asked for
    if (seg_order != 2) std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &x, const Chunk &y) { return x.end - x.beg > y.end - y.beg; });
    out->n_chunks = (int32_t)chunks.size();
    out->n_long = (int32_t)longs.size();
    if (chunks.empty() && longs.empty()) return MI_SPMM_OK;
    const size_t cb = chunks.size() * sizeof(Chunk), lb = longs.size() * sizeof(LongRow);
    if (hipMalloc((void **)&out->d_chunks, cb ? cb : sizeof(Chunk)) != hipSuccess || hipMalloc((void **)&out->d_long, lb ? lb : sizeof(LongRow)) != hipSuccess)
        return MI_SPMM_ENOMEM;
    if (cb) HIP_TRY(hipMemcpy(out->d_chunks, chunks.data(), cb, hipMemcpyHostToDevice));
    if (lb) HIP_TRY(hipMemcpy(out->d_long, longs.data(), lb, hipMemcpyHostToDevice));
    return MI_SPMM_OK;
}

// The plan tables for one hub threshold (0 = auto) and one medium threshold (0 = auto), from the builder "gpu_preprocess" selects, then the column strips
// of their segments.
static int build_tables(mi_spmm_handle *h, int64_t thr, int64_t mthr_want)
{
    const int32_t mthr = (int32_t)((thr == 0 || mthr_want < thr) ? mthr_want : thr);
    const unsigned int *d_bad = h->nnz > 0 ? h->d_col_bad : nullptr;
    PlanOut po;
    const int rc = h->gpu_preprocess
        ? build_plan_gpu(h->d_ptr, h->d_idx, h->num_v, h->num_cols, h->feat, h->nnz, h->d_blk_flag, d_bad, mthr, (int32_t)thr, (int32_t)h->long_chunk,
                         (int32_t)h->split_long, (int32_t)h->in_force.seg_order, &h->scratch_a, &h->scratch_b, &po)
        : build_plan_host(h->d_ptr, h->d_idx, h->num_v, h->num_cols, h->feat, h->nnz, h->d_blk_flag, d_bad, mthr, (int32_t)thr, (int32_t)h->long_chunk,
                          (int32_t)h->split_long, (int32_t)h->in_force.seg_order, h->d_col_bad ? (char *)h->d_col_bad + 64 : nullptr, &po);
    h->d_chunks = po.d_chunks;
    h->d_long = po.d_long;
    h->d_blk_groups = po.d_blk_groups;
    if (rc != 0) return rc;
    h->n_chunks = po.n_chunks;
    h->n_long = po.n_long;
    h->n_slots = po.n_slots;
    h->n_medium = po.n_medium;
    h->n_blk_groups = po.n_blk_groups;
    h->max_row_nnz = po.max_len;
    h->medium_res = po.mthr;
    h->long_thr = po.thr;
    h->local_pct = po.local_pct;
    h->front_pct = po.front_pct;
    h->seg_nnz = po.seg_nnz;
    return plan_col_strips(h);
}

// Drops the segment, hub and block-group tables of a plan that is built again (the block flags stay: detection does not depend on the plan).
static void drop_tables(mi_spmm_handle *h)
{
    if (h->d_chunks) (void)hipFree(h->d_chunks);
    if (h->d_long) (void)hipFree(h->d_long);
    if (h->d_blk_groups) (void)hipFree(h->d_blk_groups);
    h->d_chunks = nullptr;
    h->d_long = nullptr;
    h->d_blk_groups = nullptr;
    h->ws_bytes = 0;
}

// What the plan just built asks for, once its strips are known.
enum class Rebuild { kKeep, kFoldHubs, kKeepRows, kUnfold };
static int32_t keep_rows_to(const mi_spmm_handle *h) { return h->feat >= 128 ? 1024 : 512; }
static Rebuild next_plan(const mi_spmm_handle *h, bool folded)
{
    // The fold lost its strips (the folded plan surveys the former hub rows for the first time; if one of them has non-ascending columns, or the
    // rule on the new survey says no strips, a 10^4-nonzero row would run as ONE unstripped segment chain): back to the plan with hubs, this time to be kept.
    if (folded) return h->n_strips <= 1 ? Rebuild::kUnfold : Rebuild::kKeep;
    const Tunables &f = h->in_force;
    const int32_t M = h->num_v;
    // Strips in force and a hub threshold that was ours to choose: a plan WITHOUT hubs when the longest row's sub-chains would hide inside the strips'
    // launches -- as stripped segments those rows gather out of L2 like the rest, where the hub kernel gathers them out of all of B beside the strip
    // launches (reddit-shaped N = 128 / 256: 5.07 -> 4.46, 8.97 -> 8.15 ms).  The longest row's chain, at 100 ns per nonzero over all strips, has to fit
    // into half of the stripped step's estimate: at N = 32 the same graph's 20 758-nonzero row would be the step (1.08 -> 1.70 ms) and protein-shaped
    // N = 32 loses 7 % (0.72 -> 0.78): both keep their hubs.  profiles/r04_col_strips.txt section 8
    constexpr double kStrippedRate = 12e12;     // a stripped step: about twice the gather model's rate
    const double step_s = gather_bytes(h->nnz, M, h->feat) / kStrippedRate;
    if (f.hub_thr == 0 && !h->split_long && h->n_strips > 1 && h->n_long > 0 && (double)h->max_row_nnz * 100e-9 <= 0.5 * step_s) return Rebuild::kFoldHubs;
    // Local columns, a wide B, segments that hold a quarter of the nonzeros and NO strips for them (columns out of order, or B beyond the rule): what is left
    // to them is the length-sorted table that scatters neighbours -- the rows kernel takes them instead, up to 1 024 nonzeros (protein-unsorted N = 128 / 256:
    // 0.83 - 0.85 of the time; profiles/r05_regret.md).  One more plan: ~0.3 ms of preprocess.
    // (narrow B: up to 512 -- protein-unsorted kLen 32: 0.85 -- and only on graphs whose ROWS are long, mean degree >= 64: citation-community, mean 10, lost 17 % with it)
    if (f.medium_thr == 0 && !h->split_long && h->local_pct >= 50 && h->local_pct < 95 && M >= 65536 && h->n_strips <= 1 && h->medium_res < keep_rows_to(h) &&
        h->seg_nnz * 4 >= h->nnz && (h->feat >= 128 || h->nnz / M >= 64))
        return Rebuild::kKeepRows;
    return Rebuild::kKeep;
}

// The plan half of preprocess (mi_spmm_preprocess adds the tuner).  One sequence for both plan builders: hub threshold, column check, block detection,
// the tables (device or host builder) and their strips, the post-build decision (at most one rebuild, plus the unfold fallback), partial sums, block
// items, side streams.  The column check only launches here; the builder reads its flag back and rejects the CSR before any table is used (block
// detection runs on an unvalidated row_ptr: detect_row_blocks keeps its own reads inside [0, nnz)).
static int preprocess_plan(mi_spmm_handle *h)
{
    if (!good(h)) return MI_SPMM_ESTATE;
    const auto t0 = std::chrono::steady_clock::now();
    free_plan(h);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MI_SPMM_ENODEVICE;
    const int32_t M = h->num_v;
    auto tp = t0;
    auto lap = [&](int i) {
        const auto now = std::chrono::steady_clock::now();
        h->phase_us[i] = std::chrono::duration<double, std::micro>(now - tp).count();
        tp = now;
    };
    const int64_t thr = hub_threshold_for(h, h->in_force.hub_thr);
    h->long_thr = thr;
    if (!h->d_col_bad) HIP_TRY(hipMalloc((void **)&h->d_col_bad, 256));     // column-range flag; the 192 bytes behind it: column sample, strip survey
    lap(0);
    // column range: one pass over col_idx on the device (an out-of-range column is an out-of-bounds read of B, i.e. a GPU fault)
    if (h->nnz > 0) {
        hipError_t e = hipMemsetAsync(h->d_col_bad, 0, sizeof(unsigned int), 0);
        if (e == hipSuccess) {
            const int64_t want = (h->nnz + kBlockThreads * 8 - 1) / (kBlockThreads * 8);
            const int grid = (int)(want < 1 ? 1 : (want > 4096 ? 4096 : want));
            hipLaunchKernelGGL(csr_check_cols, dim3(grid), dim3(kBlockThreads), 0, 0, h->d_idx, h->nnz, h->num_cols, h->d_col_bad);
            e = hipGetLastError();
        }
        if (e != hipSuccess) return (int)e;
    }
    lap(1);
    // block path: 16-row groups with one shared column list (min_len <= L <= detection cap).  A group's list may be as long as the longest exact segment
    // (auto hub threshold: at most its largest candidate).
    if (h->block_path && !h->ftz && block_path_shape_ok(h->feat) && M >= 16 && h->nnz > 0) {
        const int32_t n_groups = (M + 15) / 16;
        if (hipMalloc((void **)&h->d_blk_flag, (size_t)n_groups) != hipSuccess) return MI_SPMM_ENOMEM;
        hipLaunchKernelGGL(detect_row_blocks, dim3((n_groups + 3) / 4), dim3(kBlockThreads), 0, 0, h->d_ptr, h->d_idx, M, (int32_t)h->nnz,
                           (int32_t)h->block_min_len, (int32_t)(thr > 0 ? thr : hist_threshold(kHistN - 1)), h->d_blk_flag);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { free_plan(h); return (int)e; }
    }
    lap(2);
    int rc = build_tables(h, thr, h->in_force.medium_thr);
    const Rebuild next = rc == 0 ? next_plan(h, false) : Rebuild::kKeep;
    if (next == Rebuild::kFoldHubs) {
        drop_tables(h);
        rc = build_tables(h, hub_threshold_for(h, 1 << 30), h->in_force.medium_thr);     // every row up to any length: one exact segment (stripped)
        if (rc == 0 && next_plan(h, true) == Rebuild::kUnfold) {
            drop_tables(h);
            rc = build_tables(h, thr, h->in_force.medium_thr);
        }
    } else if (next == Rebuild::kKeepRows) {
        drop_tables(h);
        rc = build_tables(h, thr, keep_rows_to(h));
    }
    if (rc != 0) { free_plan(h); return rc; }
    if (h->n_blk_groups == 0 && h->d_blk_flag) { (void)hipFree(h->d_blk_flag); h->d_blk_flag = nullptr; }
    h->n_rows_for_rows_kernel = (int64_t)M - 16 * (int64_t)h->n_blk_groups - (int64_t)h->n_long - (int64_t)h->n_medium;
    h->ldp = ((int64_t)h->feat + 3) / 4 * 4;
    lap(3);
    if (h->n_slots > 0) {
        const size_t pb = (size_t)h->n_slots * (size_t)h->ldp * sizeof(float);
        if (hipMalloc((void **)&h->d_partials, pb) != hipSuccess) { free_plan(h); return MI_SPMM_ENOMEM; }
        h->ws_bytes += pb;
    }
    h->ws_bytes += (size_t)h->n_chunks * sizeof(Chunk) + (size_t)h->n_long * sizeof(LongRow);
    rc = build_block_items(h);
    lap(4);
    if (rc == 0) rc = ensure_side_streams(h);
    if (rc == 0) rc = note_hub_rows(h);
    if (rc != 0) { free_plan(h); return rc; }
    // mi_spmm.h: preprocess synchronises.  Everything above ran on the null stream and most of it was waited for by the copies back, but the last
    // launches (build_col_strips, the block items' device copy) were not: a run() on a non-blocking stream is not ordered behind the null stream.
    HIP_TRY(hipStreamSynchronize(0));
    h->prepared = true;
    h->preprocess_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return MI_SPMM_OK;
}

extern "C" {

int mi_spmm_abi_version(void) { return MI_SPMM_ABI_VERSION; }

const char *mi_spmm_build_info(void)
{
    return "mi_spmm gfx950 (CDNA4) hand-written HIP; abi "
#define MI_STR2(x) #x
#define MI_STR(x) MI_STR2(x)
        MI_STR(MI_SPMM_ABI_VERSION) "; hip " MI_STR(HIP_VERSION_MAJOR) "." MI_STR(HIP_VERSION_MINOR);
}

const char *mi_spmm_strerror(int code)
{
    switch (code) {
    case MI_SPMM_OK: return "ok";
    case MI_SPMM_EINVAL: return "mi_spmm: invalid argument";
    case MI_SPMM_ENOMEM: return "mi_spmm: out of memory";
    case MI_SPMM_ESTATE: return "mi_spmm: bad handle or run() before preprocess()";
    case MI_SPMM_ECSR: return "mi_spmm: malformed CSR (row_ptr not monotone, row_ptr[M] != nnz, or column out of range)";
    case MI_SPMM_EUNSUPPORTED: return "mi_spmm: unsupported option or shape";
    case MI_SPMM_ENODEVICE: return "mi_spmm: no usable HIP device";
    default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "mi_spmm: unknown error";
}

int mi_spmm_create(mi_spmm_handle **out, const int32_t *d_row_ptr, const int32_t *d_col_idx,
                   const float *d_vals, int32_t num_v, int32_t num_cols, int64_t nnz, int32_t feat_in)
{
    if (!out) return MI_SPMM_EINVAL;
    *out = nullptr;
    if (num_v < 0 || num_cols < 0 || nnz < 0 || feat_in < 0) return MI_SPMM_EINVAL;
    if (nnz > INT32_MAX) return MI_SPMM_EUNSUPPORTED;  // int32 row_ptr cannot address more
    if (!d_row_ptr) return MI_SPMM_EINVAL;
    if (nnz > 0 && (!d_col_idx || !d_vals)) return MI_SPMM_EINVAL;
    mi_spmm_handle *h = new (std::nothrow) mi_spmm_handle();
    if (!h) return MI_SPMM_ENOMEM;
    std::memset(h, 0, sizeof(*h));
    h->magic = kMagic;
    h->d_ptr = d_row_ptr;
    h->d_idx = d_col_idx;
    h->d_val = d_vals;
    h->num_v = num_v;
    h->num_cols = num_cols;
    h->nnz = nnz;
    h->feat = feat_in;
    // the tuner's seven: auto, resolved in preprocess and run (fused_step 2 = auto: run_part, short steps only)
    h->user = Tunables{0, 0, 0, 0, 2, 0, 0};
    h->in_force = h->user;
    h->long_thr = 0;
    h->split_long = 0;     // every row one chain in stored order (the reference's definition, spmm_ref.cu:10-14)
    h->hub_slice = 0;
    h->hub_overlap = 1;
    h->side_priority = 3;
    h->segment_overlap = 2;   // auto: a side stream for the segment kernel only where its longest chains are long (ensure_side_streams)
    h->long_chunk = 256;   // the reference's kBatchSize (spmm_opt.cu:6)
    h->rows_per_block = 0; // auto: one row per lane group (measured best at every N, profiles/r01_sweeps)
    h->xcd_remap = -1;     // auto (see run)
    h->nt_store = 1;       // C is write-once
    h->nt_stream = 0;      // (col,val) fetches straddle lines: nt would drop the line before its other half is used
    h->block_path = 1;
    h->block_min_len = 8;
    h->block_share = 2;
    h->block_max_pieces = kMaxPieces;
    h->block_run_min = 32;
    h->block_wg_waves = 1;
    h->kernel = 2;
    h->gpu_preprocess = 1;
    h->block_threads = 256;
    h->split_cols = 1;
    h->fused_order = 0;     // auto (run_part: the role whose longest chain lasts longest goes first)
    h->n_strips = 1;
    h->seg_unsorted = -1;
    h->segment_unroll = 0;  // auto: 32 (the whole 32-pair item in flight: 0-13 % faster than 8 on every shape, profiles/r01_segment_unroll.txt) -- 16 for
                            // column-strip launches (gathers served by L2 return sooner, occupancy buys more: -2 .. -13 %, profiles/r04_col_strips.txt)
    *out = h;
    return MI_SPMM_OK;
}

int mi_spmm_set_feat(mi_spmm_handle *h, int32_t feat_in)
{
    if (!good(h) || feat_in < 0) return MI_SPMM_EINVAL;
    if (feat_in != h->feat) {
        h->feat = feat_in;
        free_plan(h);
    }
    return MI_SPMM_OK;
}

int mi_spmm_destroy(mi_spmm_handle *h)
{
    if (!h) return MI_SPMM_OK;
    if (!good(h)) return MI_SPMM_ESTATE;
    free_plan(h);
    scratch_release(&h->scratch_a);
    scratch_release(&h->scratch_b);
    if (h->d_col_bad) (void)hipFree(h->d_col_bad);
    if (h->d_blk_items) (void)hipFree(h->d_blk_items);
    if (h->d_strips) (void)hipFree(h->d_strips);
    for (int i = 0; i < 2; ++i) {
        if (h->side[i]) (void)hipStreamDestroy(h->side[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    h->magic = 0;
    delete h;
    return MI_SPMM_OK;
}

int mi_spmm_set_option(mi_spmm_handle *h, const char *key, int64_t v)
{
    if (!good(h) || !key) return MI_SPMM_EINVAL;
    const std::string k(key);
    if (k == "use_graph") return MI_SPMM_EUNSUPPORTED;      // removed in round 5 (it only ever lost: profiles/r05_use_graph_experiment.md); a caller captures run() itself
    // (the tuner's seven settings: set_option writes both copies, so that the keys that keep the plan take effect on the next run)
    else if (k == "medium_row_threshold") { if (v < 0) return MI_SPMM_EINVAL; h->user.medium_thr = h->in_force.medium_thr = v > INT32_MAX ? INT32_MAX : v; free_plan(h); }
    else if (k == "long_row_threshold") { if (v < 0) return MI_SPMM_EINVAL; h->user.hub_thr = h->in_force.hub_thr = h->long_thr = v > INT32_MAX ? INT32_MAX : v; free_plan(h); }
    else if (k == "split_long_rows") { h->split_long = v ? 1 : 0; free_plan(h); }
    else if (k == "hub_slice") { if (v != 0 && v != 16 && v != 32 && v != 64) return MI_SPMM_EINVAL; h->hub_slice = v; }
    else if (k == "hub_overlap") { if (v < 0 || v > 2) return MI_SPMM_EINVAL; h->hub_overlap = v; free_plan(h); }
    else if (k == "segment_overlap") { if (v < 0 || v > 2) return MI_SPMM_EINVAL; h->segment_overlap = v; free_plan(h); }
    else if (k == "flush_denormals") { h->ftz = v ? 1 : 0; free_plan(h); }       // (the block path is not used with it: preprocess again)
    else if (k == "side_priority") {
        if (v < 0 || v > 3) return MI_SPMM_EINVAL;
        if (v != h->side_priority) {          // the streams are made by the next preprocess
            for (int i = 0; i < 2; ++i) {
                if (h->side[i]) { (void)hipStreamSynchronize(h->side[i]); (void)hipStreamDestroy(h->side[i]); h->side[i] = nullptr; }
                if (h->ev_join[i]) { (void)hipEventDestroy(h->ev_join[i]); h->ev_join[i] = nullptr; }
            }
            if (h->ev_fork) { (void)hipEventDestroy(h->ev_fork); h->ev_fork = nullptr; }
        }
        h->side_priority = v;
        free_plan(h);
    }
    else if (k == "long_row_chunk") { if (v < 1 || v > kMaxLongChunk) return MI_SPMM_EINVAL; h->long_chunk = v; free_plan(h); }
    else if (k == "rows_per_block") { if (v < 0 || v > (1 << 20)) return MI_SPMM_EINVAL; h->rows_per_block = v; }
    else if (k == "xcd_remap") h->xcd_remap = v < 0 ? -1 : (v ? 1 : 0);
    else if (k == "kernel") {
        if (v == 1) return MI_SPMM_EUNSUPPORTED;   // the first-generation rows kernel was retired in round 3 (git history: 0894343)
        if (v != 2) return MI_SPMM_EINVAL;
        h->kernel = v;
    }
    else if (k == "gpu_preprocess") { h->gpu_preprocess = v ? 1 : 0; free_plan(h); }
    else if (k == "split_cols") h->split_cols = v ? 1 : 0;
    else if (k == "tile_cols") { if (v != 0 && v != 32 && v != 64 && v != 128 && v != 256) return MI_SPMM_EINVAL; h->user.tile_cols = h->in_force.tile_cols = v; }
    else if (k == "segment_unroll") { if (v != 0 && v != 8 && v != 16 && v != 32) return MI_SPMM_EINVAL; h->segment_unroll = v; }
    else if (k == "col_strips") { if (v < 0 || v > kMaxColStrips) return MI_SPMM_EINVAL; h->user.col_strips = h->in_force.col_strips = v; free_plan(h); }
    else if (k == "fused_step") { if (v < 0 || v > 2) return MI_SPMM_EINVAL; h->user.fused_step = h->in_force.fused_step = v; }
    else if (k == "fused_order") { if (v < 0 || v > 2) return MI_SPMM_EINVAL; h->fused_order = v; }
    else if (k == "segment_order") { if (v < 0 || v > 2) return MI_SPMM_EINVAL; h->user.seg_order = h->in_force.seg_order = v; free_plan(h); }
    else if (k == "autotune") { if (v != 0 && v != 1) return MI_SPMM_EINVAL; h->autotune = v; free_plan(h); }
    else if (k == "rows_unroll") { if (v != 0 && v != 8 && v != 16) return MI_SPMM_EINVAL; h->user.rows_unroll = h->in_force.rows_unroll = v; }
    else if (k == "col_strips_builder") { if (v != 0 && v != 1) return MI_SPMM_EINVAL; h->strips_builder = v; free_plan(h); }
    else if (k == "block_threads") { if (v != 64 && v != 128 && v != 256) return MI_SPMM_EINVAL; h->block_threads = v; }
    else if (k == "nt_store") h->nt_store = v ? 1 : 0;
    else if (k == "nt_stream") h->nt_stream = v ? 1 : 0;
    else if (k == "block_path") { h->block_path = v ? 1 : 0; free_plan(h); }
    else if (k == "block_min_len") { if (v < 1) return MI_SPMM_EINVAL; h->block_min_len = v; free_plan(h); }
    else if (k == "block_share") { if (v < 1 || v > kMaxShare) return MI_SPMM_EINVAL; h->block_share = v; free_plan(h); }
    else if (k == "block_max_pieces") { if (v < 1 || v > kMaxPieces) return MI_SPMM_EINVAL; h->block_max_pieces = v; free_plan(h); }
    else if (k == "block_wg_waves") { if (v != 1 && v != 2 && v != 4) return MI_SPMM_EINVAL; h->block_wg_waves = v; }
    else if (k == "block_run_min") { if (v < 1) return MI_SPMM_EINVAL; h->block_run_min = v > INT32_MAX ? INT32_MAX : v; free_plan(h); }
    else return MI_SPMM_EUNSUPPORTED;
    return MI_SPMM_OK;
}

int mi_spmm_get_option(const mi_spmm_handle *h, const char *key, int64_t *value)
{
    if (!good(h) || !key || !value) return MI_SPMM_EINVAL;
    const std::string k(key);
    if (k == "long_row_threshold") *value = h->long_thr;
    else if (k == "medium_row_threshold") *value = h->prepared ? h->medium_res : h->in_force.medium_thr;
    else if (k == "n_medium_rows") *value = h->n_medium;
    else if (k == "n_partial_slots") *value = h->n_slots;
    else if (k == "long_row_chunk") *value = h->long_chunk;
    else if (k == "split_long_rows") *value = h->split_long;
    else if (k == "hub_slice") *value = h->hub_slice;
    else if (k == "hub_overlap") *value = h->hub_overlap;
    else if (k == "side_priority") *value = h->side_priority;
    else if (k == "side_stream_overlaps") *value = h->side[0] ? h->side_overlaps[0] : -1;
    else if (k == "segment_overlap") *value = h->segment_overlap;
    else if (k == "flush_denormals") *value = h->ftz;
    else if (k == "n_hub_rows") *value = h->split_long ? 0 : h->n_long;
    else if (k == "rows_per_block") *value = h->rows_per_block;
    else if (k == "xcd_remap") *value = h->xcd_remap;
    else if (k == "kernel") *value = h->kernel;
    else if (k == "gpu_preprocess") *value = h->gpu_preprocess;
    else if (k == "block_threads") *value = h->block_threads;
    else if (k == "segment_unroll") *value = h->segment_unroll;
    else if (k == "split_cols") *value = h->split_cols;
    else if (k == "tile_cols") *value = h->in_force.tile_cols;
    else if (k == "nt_store") *value = h->nt_store;
    else if (k == "nt_stream") *value = h->nt_stream;
    else if (k == "block_path") *value = h->block_path;
    else if (k == "n_long_rows") *value = h->n_long;
    else if (k == "n_chunks") *value = h->n_chunks;
    else if (k == "col_strips") *value = h->in_force.col_strips;
    else if (k == "n_col_strips") *value = h->n_strips;
    else if (k == "segments_unsorted") *value = h->seg_unsorted;
    else if (k == "col_strips_builder") *value = h->strips_builder;
    else if (k == "fused_step") *value = h->in_force.fused_step;
    else if (k == "segment_order") *value = h->in_force.seg_order;
    else if (k == "autotune") *value = h->autotune;
    else if (k == "rows_unroll") *value = h->in_force.rows_unroll;
    else if (k == "autotune_evals") *value = h->tune_evals;
    else if (k == "autotune_auto_us") *value = (int64_t)(h->tune_auto_ms * 1e3);
    else if (k == "autotune_best_us") *value = (int64_t)(h->tune_best_ms * 1e3);
    else if (k == "autotune_mask") *value = tuned_settings(h->user, h->in_force);
    else if (k == "fused_step_in_force") *value = h->last_fused;
    else if (k == "fused_order") *value = h->fused_order;
    else if (k == "rows_unroll_in_force") *value = h->last_rows_deep ? 16 : 8;
    else if (k == "fused_order_in_force") *value = h->last_fused ? (h->last_seg_first ? 2 : 1) : 0;
    else if (k == "segment_nnz") *value = h->seg_nnz;
    else if (k == "col_strips_table_hash") {           // FNV-1a over the strip tables (copied back: a test's question, not a step's)
        *value = 0;
        if (h->prepared && h->d_strips && h->n_strips > 1) {
            std::vector<Chunk> t((size_t)h->n_strips * (size_t)h->n_chunks);
            HIP_TRY(hipMemcpy(t.data(), h->d_strips, t.size() * sizeof(Chunk), hipMemcpyDeviceToHost));
            uint64_t f = 1469598103934665603ull;
            const unsigned char *b = reinterpret_cast<const unsigned char *>(t.data());
            for (size_t i = 0; i < t.size() * sizeof(Chunk); ++i) { f ^= b[i]; f *= 1099511628211ull; }
            *value = (int64_t)(f >> 1);
        }
    }
    else if (k == "workspace_bytes") *value = (int64_t)(h->ws_bytes + h->scratch_a.cap + h->scratch_b.cap);   // plan tables + partial sums + the two preprocess arenas (kept until destroy)
    else if (k == "feat") *value = h->feat;
    else if (k == "num_v") *value = h->num_v;
    else if (k == "num_cols") *value = h->num_cols;
    else if (k == "max_row_nnz") *value = h->max_row_nnz;
    else if (k == "column_locality_pct") *value = h->local_pct;
    else if (k == "column_front_pct") *value = h->front_pct;
    else if (k == "n_launches") *value = h->last_launches;
    else if (k == "lanes_per_row") *value = h->last_lpr;
    else if (k == "vector_width") *value = h->last_v;
    else if (k == "wide_addressing") *value = h->last_wide;
    else if (k == "n_block_groups") *value = h->n_blk_groups;
    else if (k == "block_min_len") *value = h->block_min_len;
    else if (k == "block_share") *value = h->block_share;
    else if (k == "block_max_pieces") *value = h->block_max_pieces;
    else if (k == "block_run_min") *value = h->block_run_min;
    else if (k == "block_wg_waves") *value = h->block_wg_waves;
    else if (k == "n_block_items") *value = h->n_blk_items;
    else if (k == "n_block_pieces") *value = h->n_blk_pieces;
    else if (k == "n_block_passes") *value = h->n_blk_passes;
    else if (k == "n_block_shared_items") *value = h->n_blk_shared_items;
    else if (k == "preprocess_us") *value = (int64_t)h->preprocess_us;
    else if (k == "pre_d2h_us") *value = (int64_t)h->phase_us[0];
    else if (k == "pre_colcheck_us") *value = (int64_t)h->phase_us[1];
    else if (k == "pre_detect_us") *value = (int64_t)h->phase_us[2];
    else if (k == "pre_table_us") *value = (int64_t)h->phase_us[3];
    else if (k == "pre_upload_us") *value = (int64_t)h->phase_us[4];
    else if (k == "prepared") *value = h->prepared ? 1 : 0;
    else return MI_SPMM_EUNSUPPORTED;
    return MI_SPMM_OK;
}

}  // extern "C"

// ---- launch dispatch ------------------------------------------------------------
namespace {


// v2 rows kernel: the cache policy (nt C stores x nt (col,val) loads) and the workgroup size are
// instantiated for the 16-byte narrow path, which every benchmark shape uses; the dword and
// wide-address fallbacks get the default policy.
template <int LPR, int BT>
void launch_rows_v2_pol(int pol, const RowsArgs &a, dim3 grid, hipStream_t s)
{
    switch (pol & 3) {
    case 0: hipLaunchKernelGGL((spmm_rows_v2<4, LPR, 8, false, 0, BT>), grid, dim3(BT), 0, s, a); break;
    case 1: hipLaunchKernelGGL((spmm_rows_v2<4, LPR, 8, false, 1, BT>), grid, dim3(BT), 0, s, a); break;
    case 2: hipLaunchKernelGGL((spmm_rows_v2<4, LPR, 8, false, 2, BT>), grid, dim3(BT), 0, s, a); break;
    default: hipLaunchKernelGGL((spmm_rows_v2<4, LPR, 8, false, 3, BT>), grid, dim3(BT), 0, s, a); break;
    }
}
template <int LPR>
void launch_rows_v2_bt(int bt, int pol, const RowsArgs &a, dim3 grid, hipStream_t s)
{
    if (bt == 64) launch_rows_v2_pol<LPR, 64>(pol, a, grid, s);
    else if (bt == 128) launch_rows_v2_pol<LPR, 128>(pol, a, grid, s);
    else launch_rows_v2_pol<LPR, 256>(pol, a, grid, s);
}
// The default cache policy and 256-thread workgroups at a fixed depth: the dword and wide-address fallbacks (8 deep) and
// "rows_unroll" = 16: sixteen gathers in flight per lane group (default cache policy, 256-thread workgroups only).  Half the round trips per row at two
// thirds of the occupancy: -13 % ... +23 % by graph (profiles/r05_rows_unroll_ab.txt), so never the rule's choice; "autotune" tries it
template <int V, int UNROLL, bool WIDE>
void launch_rows_v2_fixed(int lpr, const RowsArgs &a, dim3 grid, hipStream_t s)
{
    switch (lpr) {
    case 8: hipLaunchKernelGGL((spmm_rows_v2<V, 8, UNROLL, WIDE, 1, 256>), grid, dim3(256), 0, s, a); break;
    case 16: hipLaunchKernelGGL((spmm_rows_v2<V, 16, UNROLL, WIDE, 1, 256>), grid, dim3(256), 0, s, a); break;
    case 32: hipLaunchKernelGGL((spmm_rows_v2<V, 32, UNROLL, WIDE, 1, 256>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((spmm_rows_v2<V, 64, UNROLL, WIDE, 1, 256>), grid, dim3(256), 0, s, a); break;
    }
}
// deep: the 16-deep instance (16-byte narrow lanes, 256 threads, kPolNtStore only: rows_deep)
void launch_rows_v2_any(bool vec4, bool wide, bool deep, int lpr, int bt, int pol, const RowsArgs &a, dim3 grid, hipStream_t s)
{
    if (deep) launch_rows_v2_fixed<4, 16, false>(lpr, a, grid, s);
    else if (vec4 && !wide) {
        switch (lpr) {
        case 8: launch_rows_v2_bt<8>(bt, pol, a, grid, s); break;
        case 16: launch_rows_v2_bt<16>(bt, pol, a, grid, s); break;
        case 32: launch_rows_v2_bt<32>(bt, pol, a, grid, s); break;
        default: launch_rows_v2_bt<64>(bt, pol, a, grid, s); break;
        }
    } else if (vec4) launch_rows_v2_fixed<4, 8, true>(lpr, a, grid, s);
    else if (wide) launch_rows_v2_fixed<1, 8, true>(lpr, a, grid, s);
    else launch_rows_v2_fixed<1, 8, false>(lpr, a, grid, s);
}

template <int V, int LPR, bool WIDE>
void launch_chunks(const ChunkArgs &a, dim3 grid, hipStream_t s, int deep)
{
    // deep = gathers in flight per lane group (16-byte narrow path; the fallbacks keep 8).  A segment is one
    // long dependent chain per lane group, so more loads in flight is what buys speed; 32 = a whole item.
    if (deep == 32 && V == 4 && !WIDE) hipLaunchKernelGGL((spmm_chunks<V, LPR, 32, false>), grid, dim3(kBlockThreads), 0, s, a);
    else if (deep == 16 && V == 4 && !WIDE) hipLaunchKernelGGL((spmm_chunks<V, LPR, 16, false>), grid, dim3(kBlockThreads), 0, s, a);
    else hipLaunchKernelGGL((spmm_chunks<V, LPR, 8, WIDE>), grid, dim3(kBlockThreads), 0, s, a);
}
template <int V, bool WIDE>
void launch_chunks_lpr(int lpr, const ChunkArgs &a, dim3 grid, hipStream_t s, int deep)
{
    switch (lpr) {
    case 8: launch_chunks<V, 8, WIDE>(a, grid, s, deep); break;
    case 16: launch_chunks<V, 16, WIDE>(a, grid, s, deep); break;
    case 32: launch_chunks<V, 32, WIDE>(a, grid, s, deep); break;
    default: launch_chunks<V, 64, WIDE>(a, grid, s, deep); break;
    }
}
// [vec4][wide]
constexpr void (*kLaunchChunks[2][2])(int, const ChunkArgs &, dim3, hipStream_t, int) = {
    {launch_chunks_lpr<1, false>, launch_chunks_lpr<1, true>}, {launch_chunks_lpr<4, false>, launch_chunks_lpr<4, true>}};

template <int G, bool WIDE, bool RUN>
void launch_block_items_g(int slab, const BlockArgs &a, dim3 grid, hipStream_t s, int bt)
{
    // slab = columns one wave covers: 256 / 128 / 64 as 4 / 2 / 1 chunks of 64 (16 bytes per lane), 32 as one chunk of
    // 32 (8 bytes per lane).  Shared items (G > 1) exist only for 256 and 128 (N % 128 == 0).
    if (slab == 256) hipLaunchKernelGGL((spmm_block_items<4, 4, G, WIDE, RUN>), grid, dim3(bt), 0, s, a);
    else if (slab == 128) hipLaunchKernelGGL((spmm_block_items<2, 4, G, WIDE, RUN>), grid, dim3(bt), 0, s, a);
    else if (G == 1 && slab == 64) hipLaunchKernelGGL((spmm_block_items<1, 4, 1, WIDE, RUN>), grid, dim3(bt), 0, s, a);
    else if (G == 1) hipLaunchKernelGGL((spmm_block_items<1, 2, 1, WIDE, RUN>), grid, dim3(bt), 0, s, a);
}
// [cls][wide]; cls: 0 = list items, 1 = run items holding one piece, 2 = run items sharing their B rows between two pieces
constexpr void (*kLaunchBlockItems[3][2])(int, const BlockArgs &, dim3, hipStream_t, int) = {
    {launch_block_items_g<1, false, false>, launch_block_items_g<1, true, false>},
    {launch_block_items_g<1, false, true>, launch_block_items_g<1, true, true>},
    {launch_block_items_g<2, false, true>, launch_block_items_g<2, true, true>}};

void launch_small_step(int lpr, int deep, const SmallStepArgs &a, dim3 grid, hipStream_t s)
{
    // segments 16 gathers deep: 114 - 128 VGPRs beside the hub role's 112 (32 deep would make the whole kernel a 2-waves-per-SIMD kernel).  The 8-lane
    // instance is 3 dwords over 128 and spills them (12 bytes of scratch per lane); "segment_unroll" = 8 selects its 8-deep form, which does not.
    switch (lpr) {
    case 8:
        if (deep == 8) hipLaunchKernelGGL((spmm_small_step<8, 8>), grid, dim3(kBlockThreads), 0, s, a);
        else hipLaunchKernelGGL((spmm_small_step<8, 16>), grid, dim3(kBlockThreads), 0, s, a);
        break;
    case 16: hipLaunchKernelGGL((spmm_small_step<16, 16>), grid, dim3(kBlockThreads), 0, s, a); break;
    case 32: hipLaunchKernelGGL((spmm_small_step<32, 16>), grid, dim3(kBlockThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((spmm_small_step<64, 16>), grid, dim3(kBlockThreads), 0, s, a); break;
    }
}

template <bool WIDE>
void launch_hub(int sw, bool excl, const HubArgs &a, dim3 grid, hipStream_t s)
{
    if (sw == 16 && excl) hipLaunchKernelGGL((spmm_hub<16, WIDE, true>), grid, dim3(64 * (1 + HubCfg<16>::L)), 0, s, a);
    else if (sw == 16) hipLaunchKernelGGL((spmm_hub<16, WIDE>), grid, dim3(64 * (1 + HubCfg<16>::L)), 0, s, a);
    else if (sw == 64) hipLaunchKernelGGL((spmm_hub<64, WIDE>), grid, dim3(64 * (1 + HubCfg<64>::L)), 0, s, a);
    else hipLaunchKernelGGL((spmm_hub<32, WIDE>), grid, dim3(64 * (1 + HubCfg<32>::L)), 0, s, a);
}

// Column-tile width of the rows / segment kernels when the caller leaves it to us (profiles/r02_wide_n_tiles.txt; round 5: profiles/r05_regret.md):
//   columns (almost) all near the row's own position (banded / mesh, >= 95 %): whole-wave tiles -- neighbouring rows share B rows through L2 and a
//     narrower tile only re-reads A (banded N=256: 1.75 ms at 256, 1.88 at 128, 2.15 at 64);
//   community orders (50 - 94 %: most of a row near the diagonal, the rest all over B): N >= 256 -> 128-column tiles, two rows per wavefront (round 5: six
//     community-ordered dataset shapes and the plain block model at N = 256: 0.82 - 0.95 of the time with 256; the others neutral); narrower N: the whole row;
//   otherwise (columns anywhere):
//     few nonzeros per row (mean < 8: youtube-, am-, arxiv-shaped; collab-shaped, 9.7, keeps 64: 0.87): the whole row / whole-wave tiles -- a narrower tile multiplies what a ROW costs
//       (row pointers, its lane group's start, its C store) and such a row has little else (round 5: youtube-shuffled N = 128 / 256 0.83 / 0.79,
//       arxiv-degree N = 256 0.74, am-degree N = 256 0.82 of the time with 64);
//     N >= 256: 64-column tiles -- the tiles are swept one after the other, so a sweep's B working set is K x 64 x 4 bytes (256 MiB at K = 2^20: the
//       Infinity Cache's size) instead of 1 GiB (uniform N=1024: 20.3 -> 19.4 ms, N=256: 5.44 -> 4.79; R-MAT N=512: 10.3 -> 8.3; dense-ish: +6 %);
//     N < 256 with hub rows (longest row > 64 x mean: R-MAT-like column reuse): 64 as well (R-MAT N=128: 2.09 -> 1.81 ms);
//     else the whole row (uniform N=128: 2.40 at 128, 2.42 at 64, 2.57 at 32).
int resolve_tile_cols(const mi_spmm_handle *h, int32_t N)
{
    if (h->in_force.tile_cols > 0) return (int)h->in_force.tile_cols;
    if (h->local_pct < 0 || h->local_pct >= 95) return 256;
    if (h->local_pct >= 50) {
        if (N < 256) return 256;
        // (rows of a handful of nonzeros over a B far beyond the Infinity Cache -- youtube-, am-, wikikg2-community at N = 256: 0.91 - 0.94 with the whole wave)
        const int64_t mean_l = h->num_v > 0 ? h->nnz / h->num_v : 0;
        return (mean_l < 8 && 4.0 * (double)h->num_cols * (double)N > 256.0 * 1048576.0) ? 256 : 128;
    }
    // an L2-resident B (4 K N <= 6 MiB: ddi-shaped) has no working set to shrink: narrower tiles only re-read A (ddi-community N = 256: 0.76 with the whole wave)
    if (b_l2_resident(h->num_cols, N)) return 256;
    const int64_t mean = h->num_v > 0 ? h->nnz / h->num_v : 0;
    const bool hubs = (int64_t)h->max_row_nnz > 64 * (mean > 1 ? mean : 1);
    // (... except two tiles of 64 at N = 128 when the hubs come first in the vertex order: their B rows are the hot set, and half-width rows of it fit L2 --
    //  am-degree N = 128: 0.88 of the time with 64; the same graph at N = 256 prefers the whole wave by 0.82; arxiv-degree, whose B fits the Infinity Cache, 0.89 the other way)
    if (mean < 8) return (N <= 128 && N > 64 && hubs && h->front_pct >= 50 && 4.0 * (double)h->num_cols * (double)N > 256.0 * 1048576.0) ? 64 : 256;
    // (Hold-out graphs, round 5: sizing the tile so that a sweep's K x tile x 4 bytes just fit the Infinity Cache -- the whole wave once K <= 2^18 -- gains
    //  5 - 22 % on an R-MAT of scale 18 and LOSES 15 - 19 % on collab- / reddit- / protein-shaped graphs of the same K, whose strips or hub rows want the
    //  narrow tile: not adopted; profiles/r05_regret_holdout.md.)
    if (N >= 256) return 64;
    if (N >= 128 && hubs) return 64;
    return 256;
}

int pow2_ceil(int x)
{
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// narrow addressing: byte offset of any B element < 2^32, column index and
// row pitch in bytes < 2^24 (one v_mad_u32_u24 per gathered row)
bool narrow_addressing(const mi_spmm_handle *h, int64_t ldb, int32_t n)
{
    return (int64_t)h->num_cols <= (1 << 24) && ldb * 4 < (1 << 24) &&
           ((int64_t)(h->num_cols > 0 ? h->num_cols - 1 : 0) * ldb + n) * 4 <= ((int64_t)1 << 32);
}

// The step as launch_set was given it.  The hub and block kernels address its full width: they are launched with the first column part only.
struct Step {
    const float *B; float *C; int32_t N; PeerOut po;     // the caller's pointers, width and extra destinations
    int64_t ldb, ldc;
    int32_t row_begin, row_end;
    bool blocks_on;         // the MFMA block kernels can run on this call (alignment)
    hipStream_t s;
};

// One column part [col0, col0 + N) of the step and its launch shape, computed once (make_part) and read by every role's launch.
struct Part {
    int64_t col0;
    int32_t N;
    const float *B; float *C; PeerOut po;                // the step's pointers moved to column col0
    int V;                  // floats per lane: 4 or 1
    bool vec4, wide;        // wide: beyond narrow addressing
    int lpr, tile_w, col_tiles;
    int bt, rpg;            // rows kernel: workgroup size, contiguous rows per lane group
    int64_t nblk;           // rows kernel: workgroups per column tile
    int flags, pol;
};

int make_part(const mi_spmm_handle *h, const Step &st, int64_t col0, int32_t N, Part *out)
{
    Part &p = *out;
    p.col0 = col0;
    p.N = N;
    p.B = st.B + col0;
    p.C = st.C + col0;
    p.po = st.po;
    for (int q = 0; q < p.po.n; ++q) p.po.p[q] += col0;
    const int32_t M = h->num_v;
    // 16 bytes per lane whenever a row holds at least one float4: global dwordx4 accesses only need dword
    // alignment, and a row whose width is not a multiple of 4 gets its last lane shifted back to column N - 4
    // (spmm_kernels.hpp).  Only N < 4 takes the dword path.  The MFMA block path keeps the strict 16-byte rule.
    p.vec4 = N >= 4;
    p.V = p.vec4 ? 4 : 1;
    p.wide = !narrow_addressing(h, st.ldb, N);
    int lpr = pow2_ceil((N + p.V - 1) / p.V);
    if (lpr < 8) lpr = 8;
    if (lpr > 64) lpr = 64;
    // Wide B (N >= 256): the column tiles are swept one after the other (blockIdx.x runs fastest), so a tile's
    // working set is K rows x tile_cols x 4 B.  Narrower tiles keep that set nearer the Infinity Cache's size.
    const int tile_cap = resolve_tile_cols(h, N) / p.V;
    if (p.vec4 && lpr > tile_cap) lpr = tile_cap;
    p.lpr = lpr;
    p.tile_w = lpr * p.V;
    p.col_tiles = (N + p.tile_w - 1) / p.tile_w;
    p.bt = (p.vec4 && !p.wide) ? (int)h->block_threads : kBlockThreads;
    const int gpb = p.bt / lpr;
    int rpb = (int)h->rows_per_block;
    // one row per lane group -- except narrow groups on very short rows (N <= 32, mean degree < 12), where a second
    // row per group lets the next row's pairs be fetched under the current row's few gathers (+3-6 %, profiles/r01_thresholds.txt)
    const bool short_rows = lpr == 8 && M > 0 && h->nnz / M < 12;
    if (rpb <= 0) rpb = short_rows ? 2 * gpb : gpb;
    if (rpb < gpb) rpb = gpb;
    p.rpg = rpb / gpb;          // contiguous rows per lane group, at most LPR - 1
    if (p.rpg > lpr - 1) p.rpg = lpr - 1;
    if (p.rpg < 1) p.rpg = 1;
    rpb = p.rpg * gpb;
    p.nblk = ((int64_t)(st.row_end - st.row_begin) + rpb - 1) / rpb;
    if (p.nblk > INT32_MAX || p.col_tiles > 65535) return MI_SPMM_EUNSUPPORTED;
    // auto: measured neutral-to-positive everywhere except one whole-wave row and a single column
    // tile (N = 256), where interleaving rows over the XCDs is ~3 % faster (profiles/r01_sweep_*)
    const bool remap = h->xcd_remap < 0 ? !(lpr == 64 && p.col_tiles == 1) : (h->xcd_remap != 0);
    p.flags = (remap ? kFlagXcdRemap : 0) | (h->ftz ? kFlagFtz : 0);
    p.pol = (h->nt_store ? kPolNtStore : 0) | (h->nt_stream ? kPolNtStream : 0);
    return MI_SPMM_OK;
}

// ---- one argument builder per role, for the separate kernels and the small-step kernel alike ---------------------------------------------

HubArgs hub_args(const mi_spmm_handle *h, const Step &st, int slices)
{
    HubArgs a{};
    a.rows = h->d_long;
    a.row_ptr = h->d_ptr;
    a.col_idx = h->d_idx;
    a.vals = h->d_val;
    a.B = st.B;
    a.C = st.C;
    a.ldb = st.ldb;
    a.ldc = st.ldc;
    a.n_hubs = h->n_long;
    a.N = st.N;
    a.slices = slices;
    a.row_lo = st.row_begin;
    a.row_hi = st.row_end;
    a.flags = h->ftz ? kFlagFtz : 0;
    a.po = st.po;
    return a;
}

ChunkArgs segment_args(const mi_spmm_handle *h, const Step &st, const Part &p)
{
    ChunkArgs a{};
    a.chunks = h->d_chunks;
    a.col_idx = h->d_idx;
    a.vals = h->d_val;
    a.B = p.B;
    // (read only by split-row segments, slot >= 0: never in the small-step kernel, which split_long steps do not take)
    a.partials = h->d_partials + p.col0;
    a.C = p.C;
    a.ldb = st.ldb;
    a.ldp = h->ldp;
    a.ldc = st.ldc;
    a.n_chunks = h->n_chunks;
    a.N = p.N;
    a.flags = p.flags;
    a.row_lo = st.row_begin;
    a.row_hi = st.row_end;
    a.po = p.po;
    return a;
}

RowsArgs rows_args(const mi_spmm_handle *h, const Step &st, const Part &p)
{
    RowsArgs a{};
    a.blk_flag = h->n_blk_groups > 0 ? h->d_blk_flag : nullptr;
    a.row_ptr = h->d_ptr;
    a.col_idx = h->d_idx;
    a.vals = h->d_val;
    a.B = p.B;
    a.C = p.C;
    a.ldb = st.ldb;
    a.ldc = st.ldc;
    a.row0 = st.row_begin;
    a.M = st.row_end;
    a.N = p.N;
    a.rows_per_block = p.rpg;
    // rows above the medium threshold were given to the segment or hub kernel -- except rows of block groups (of any
    // length up to the detection cap): when the block path cannot run on this call (pointers or pitches not 16-byte
    // aligned) the rows kernel takes exactly those rows as well (kFlagBlockFallback), nothing is computed twice
    const bool blocks_fallback = h->n_blk_groups > 0 && !st.blocks_on;
    a.long_thr = (int32_t)h->medium_res;
    a.nblk = (int)p.nblk;
    a.flags = p.flags | (blocks_fallback ? kFlagBlockFallback : 0);
    a.po = p.po;
    return a;
}

ReduceArgs reduce_args(const mi_spmm_handle *h, const Step &st, const Part &p)
{
    ReduceArgs a{};
    a.rows = h->d_long;
    a.partials = h->d_partials + p.col0;
    a.C = p.C;
    a.ldp = h->ldp;
    a.ldc = st.ldc;
    a.n_long = h->n_long;
    a.N = p.N;
    a.flags = p.flags;
    a.row_lo = st.row_begin;
    a.row_hi = st.row_end;
    a.po = p.po;
    return a;
}

// ---- one enqueue function per role, in run_part's order ----------------------------------------------------------------------------------

// ---- small steps: one launch, three roles (spmm_kernels.hpp spmm_small_step) -------------------------------------------------------------
// Eligible: the plain case of every role -- 16-byte lanes, narrow addressing, ONE column tile, no column strips, no split rows, no block groups, the
// default workgroup size.  auto ("fused_step" = 2): only steps whose bytes take under 0.2 ms at 6 TB/s -- there the launch boundaries and the fork are
// a third of the step and the rows role's lower occupancy (3 waves per SIMD, the hub role's footprint) costs nothing; longer steps keep their kernels.
// false: nothing launched, the separate kernels take the step.
bool enqueue_small_step(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    const bool eligible = p.vec4 && !p.wide && p.col_tiles == 1 && p.N == st.N && h->n_strips <= 1 && !h->split_long && h->n_blk_groups == 0 &&
                          p.bt == kBlockThreads && p.pol == kPolNtStore && (h->n_long > 0 || h->n_chunks > 0) &&
                          (int64_t)((st.N + 15) / 16) * h->n_long + (int64_t)h->n_chunks + p.nblk < (int64_t)INT32_MAX;
    if (!eligible) return false;
    // auto: the step's bytes take under 0.1 ms, or its longest row's chain (3.2 ns per nonzero) outlasts them anyway (am-shaped): then the rows role's
    // occupancy cannot matter.  (First rule, 0.2 ms: youtube-shaped kLen 32 -- 0.155 ms of bytes, a 75 us chain, 35 K rows workgroups -- lost 6 - 14 %.)
    // (an L2-resident B -- 4 K N <= 6 MiB, ddi-shaped -- moves its bytes three times faster: priced as in plan.hpp resolve_hub_threshold)
    constexpr double kFabricRate = 6e12, kL2Rate = 18e12;
    const double t_bytes = gather_bytes(h->nnz, h->num_v, st.N) / (b_l2_resident(h->num_cols, st.N) ? kL2Rate : kFabricRate);
    // (local columns: the rows kernel alone is fast and wants its occupancy -- 0.1 ms; columns anywhere: latency-bound whatever the occupancy -- 0.16 ms:
    //  arxiv-community N = 128 loses 18 % fused, arxiv-rcm gains 16 %; youtube-community kLen 32 loses 14 %, youtube-shuffled gains 11 %)
    const double t_fused = h->local_pct >= 50 ? 100e-6 : 160e-6;
    const bool hubs_here = h->n_long > 0 && range_has_hub(h, st.row_begin, st.row_end);
    // (a step that is ONE launch anyway -- one role only: ddi-shaped N = 256, every row a segment -- keeps that role's own kernel, which is the better
    //  instance of it: segments 32 gathers deep instead of 16 at the small-step kernel's footprint; ddi-community kLen 256: 85.7 -> 79 us)
    const int n_roles = (hubs_here ? 1 : 0) + (h->n_chunks > 0 ? 1 : 0) + (h->n_rows_for_rows_kernel > 0 ? 1 : 0);
    const int64_t fused_step = h->in_force.fused_step;
    const bool want = fused_step == 1 || (fused_step == 2 && n_roles >= 2 && (t_bytes < t_fused || (double)h->max_row_nnz * 3.2e-9 > t_bytes));
    if (!want) return false;
    SmallStepArgs fa{};
    if (hubs_here) {
        fa.h = hub_args(h, st, (st.N + 15) / 16);
        fa.hub_wgs = fa.h.slices * h->n_long;
    }
    if (h->n_chunks > 0) {
        fa.c = segment_args(h, st, p);
        fa.seg_wgs = (h->n_chunks + kBlockThreads / p.lpr - 1) / (kBlockThreads / p.lpr);
    }
    fa.r = rows_args(h, st, p);
    const int rows_wgs = h->n_rows_for_rows_kernel > 0 ? (int)p.nblk : 0;       // every row may belong to the first two roles (ddi-shaped graphs)
    if (fa.hub_wgs + fa.seg_wgs + rows_wgs == 0) return false;       // (the separate kernels have nothing to launch either)
    // Which of the first two roles leads the grid (workgroups start in blockIdx order): the one whose longest chain LASTS longest.  A hub row costs
    // 3.2 ns per nonzero plus ~2 us of pipeline fill; a segment is one lane group's dependent gather chain, 47 ns per nonzero (30 out of an
    // L2-resident B), and the longest segment is as long as the hub threshold allows.  arxiv- / youtube- / am-shaped: one hub row of 10^4 - 10^5
    // nonzeros is the step -> hubs first; ddi- / collab-shaped: hub rows of 700 - 1 800 nonzeros (2 - 6 us) over 256 - 512-nonzero segments
    // (12 - 24 us) that used to START behind two rounds of hub workgroups -> segments first.
    {
        const bool l2_b = b_l2_resident(h->num_cols, st.N);
        const int64_t seg_max = h->long_thr > 0 && h->long_thr < (int64_t)h->max_row_nnz ? h->long_thr : (int64_t)h->max_row_nnz;
        const double t_seg = (double)seg_max * (l2_b ? 30e-9 : 47e-9), t_hub = 2e-6 + (double)h->max_row_nnz * 3.2e-9;
        const bool both = fa.hub_wgs > 0 && fa.seg_wgs > 0;
        fa.seg_first = both && (h->fused_order == 2 || (h->fused_order == 0 && t_seg > t_hub)) ? 1 : 0;
        h->last_seg_first = fa.seg_first;
    }
    dim3 fgrid((unsigned)(fa.hub_wgs + fa.seg_wgs + rows_wgs));
    launch_small_step(p.lpr, (int)h->segment_unroll, fa, fgrid, st.s);
    ++*launches;
    return true;
}

int enqueue_hubs(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    if (!(h->n_long > 0 && !h->split_long && p.col0 == 0 && range_has_hub(h, st.row_begin, st.row_end))) return MI_SPMM_OK;
    // the hub kernel moves 16-byte parts of B rows: its last part starts at column N - 4 (hub_threshold_for gives a narrower B no hubs)
    if (st.N < 4) return MI_SPMM_EUNSUPPORTED;
    // Slice width, when the caller leaves it to us: 32 columns per chain wave -- unless the longest row's chain alone
    // (3.3 ns per nonzero) is more than half of what the whole step's bytes take at 6 TB/s, i.e. that one chain is the
    // step: then 16, whose loaders put half as much through the LDS the chain wave reads from (am-shaped, N = 128:
    // 0.84 -> 0.72 ms; where the hub rows are many rather than one long, 32 is faster: R-MAT N = 32 0.47 vs 0.56;
    // profiles/r03_hub_experiments.txt)
    int sw = (int)h->hub_slice;
    bool excl = false;         // the chain-bound case: the hub workgroups keep their CUs to themselves (spmm_kernels.hpp EXCL)
    if (sw <= 0) {
        constexpr double kFabricRate = 6e12;
        const double step_s = gather_bytes(h->nnz, h->num_v, st.N) / kFabricRate;
        // (round 4, new chain loop: 16 and 32 are within 1-3 % of each other on chain-bound graphs up to N = 128; at N = 256 the 16 workgroups
        //  of a row cost more than they save: am-shaped 1.164 -> 1.119 ms with 32; 64 loses everywhere it is the chain that counts)
        const bool chain_bound = st.N <= 128 && (double)h->max_row_nnz * 3.3e-9 > 0.5 * step_s;
        sw = (st.N <= 16 || chain_bound) ? 16 : 32;
        // ... and only while the hub workgroups are few: each keeps a whole CU, and 184 hubs x 8 slices of them (am-community N = 128) held the chip
        // until the last one had gone -- the rows kernel behind them started late: 0.43 -> 0.57 ms (profiles/r05_regret.md)
        excl = chain_bound && (int64_t)((st.N + 15) / 16) * h->n_long <= 128;
    }
    const int slices = (st.N + sw - 1) / sw;
    if ((int64_t)slices * h->n_long > INT32_MAX) return MI_SPMM_EUNSUPPORTED;
    hipStream_t hs;
    if (const int fr = side_stream(h, 0, st.s, &hs)) return fr;
    dim3 hgrid((unsigned)(slices * h->n_long));
    (narrow_addressing(h, st.ldb, st.N) ? launch_hub<false> : launch_hub<true>)(sw, excl, hub_args(h, st, slices), hgrid, hs);
    ++*launches;
    return MI_SPMM_OK;
}

int enqueue_segments(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    if (h->n_chunks <= 0) return MI_SPMM_OK;
    ChunkArgs ca = segment_args(h, st, p);
    const int cgpb = kBlockThreads / p.lpr;  // the chunk kernel always runs 256-thread workgroups
    dim3 cgrid((h->n_chunks + cgpb - 1) / cgpb, p.col_tiles);
    // partial rows are ldp (multiple of 4) floats and hipMalloc-aligned, so only
    // the B side decides the vector width here
    // on side stream 1: a segment is one lane group's dependent chain (up to long_row_threshold nonzeros), and the rows
    // kernel behind it in the same stream would wait for the longest one
    hipStream_t cs;
    if (const int fr = side_stream(h, 1, st.s, &cs)) return fr;
    // column strips (plan.hpp): one launch per strip in stream order, each over its own sub-segment table; every strip but the last
    // leaves the chains in the local C (plain stores, no extra destinations), the last one finishes them like an unstripped launch
    const int n_strips = (h->d_strips && h->n_strips > 1) ? h->n_strips : 1;
    for (int strip = 0; strip < n_strips; ++strip) {
        if (n_strips > 1) {
            ca.chunks = h->d_strips + (size_t)strip * (size_t)h->n_chunks;
            const bool last = strip == n_strips - 1;
            ca.flags = p.flags | (last ? (p.po.n > 0 ? kFlagStripNoSkip : 0) : kFlagStripCarry);
            if (!last) ca.po.n = 0; else ca.po = p.po;
        }
        const int deep = h->segment_unroll > 0 ? (int)h->segment_unroll : (n_strips > 1 ? 16 : 32);
        kLaunchChunks[p.vec4][p.wide](p.lpr, ca, cgrid, cs, deep);
        ++*launches;
    }
    return MI_SPMM_OK;
}

int enqueue_block_passes(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    if (!(st.blocks_on && p.col0 == 0)) return MI_SPMM_OK;
    const bool remap_blocks = h->xcd_remap != 0;   // list is column-ordered: keep neighbours on one XCD
    // the block kernel addresses the FULL width (this part may be narrower when split_cols peels a remainder)
    const bool wide_full = !narrow_addressing(h, st.ldb, st.N);
    BlockArgs ba{};
    ba.col_idx = h->d_idx;
    ba.vals = h->d_val;
    ba.B = st.B;
    ba.C = st.C;
    ba.ldb = st.ldb;
    ba.ldc = st.ldc;
    ba.N = st.N;
    ba.remap = remap_blocks ? 1 : 0;
    ba.row_lo = st.row_begin;
    ba.row_hi = st.row_end;
    ba.po = st.po;
    const int slab = block_slab_width(st.N), slabs = st.N / slab;
    // pass p continues the fma chains pass p-1 left in C: stream order is the dependency
    for (int pass = 0; pass < h->n_blk_passes; ++pass) {
        for (int cls = 2; cls >= 0; --cls) {
            int32_t n = h->blk_launch[pass][cls].n;
            ba.items = h->d_blk_items + h->blk_launch[pass][cls].off;
            if (n == 0) continue;
            ba.n_items = n;
            // one item per wave, and ONE wave per workgroup by default: items differ 4x in length (64 or 128 rows, one or two
            // pieces), and a 4-wave workgroup holds its four wave slots until its longest item is done -- 1.38 of 2 possible
            // waves per SIMD were resident against 1.80 with single-wave workgroups (profiles/r03_c4_item_timeline.txt)
            const int wpw = (int)h->block_wg_waves;
            dim3 bgrid((unsigned)((n + wpw - 1) / wpw), slabs);
            kLaunchBlockItems[cls][wide_full](slab, ba, bgrid, st.s, 64 * wpw);
            ++*launches;
        }
    }
    return MI_SPMM_OK;
}

// Gathers in flight per lane group, auto: 8 -- except where the rows kernel carries LONG rows one wave per row: banded columns (the only plans that keep
// rows of hundreds of nonzeros here: medium threshold 1 024), ONE whole-wave column tile (N = 193 ... 256: at N = 512 the second tile's wave shares the
// row's B rows and 16 gains nothing) and a mean degree >= 256.  Then a row is one wave's chain of round trips and 16 halves them: banded 300-700 rows
// 0.89 (band +-2048) / 0.90 (+-512), 600-1000 rows 0.93; mean degree 150 and below: 0.98 ... 1.06 (profiles/r05_banded_unroll_ab.jsonl)
bool rows_deep(const mi_spmm_handle *h, const Part &p)
{
    const int32_t M = h->num_v;
    const int64_t rows_unroll = h->in_force.rows_unroll;
    const bool deep_rows = rows_unroll == 16 || (rows_unroll == 0 && h->local_pct >= 95 && p.lpr == 64 && p.col_tiles == 1 && h->medium_res >= 512 &&
                                                    M > 0 && h->nnz / M >= 256);
    return deep_rows && p.vec4 && !p.wide && p.bt == kBlockThreads && p.pol == kPolNtStore;
}

int enqueue_rows(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    // every row may already be owned by the segment, split and block paths: nothing left to launch
    if ((st.blocks_on || h->n_blk_groups == 0) && h->n_rows_for_rows_kernel == 0) return MI_SPMM_OK;
    dim3 grid((unsigned)p.nblk, p.col_tiles);
    launch_rows_v2_any(p.vec4, p.wide, rows_deep(h, p), p.lpr, p.bt, p.pol, rows_args(h, st, p), grid, st.s);
    ++*launches;
    return MI_SPMM_OK;
}

int enqueue_reduce(mi_spmm_handle *h, const Step &st, const Part &p, int *launches)
{
    if (!(h->n_long > 0 && h->split_long)) return MI_SPMM_OK;
    const int64_t threads = (int64_t)h->n_long * ((p.N + p.V - 1) / p.V);
    dim3 rgrid((unsigned)((threads + kBlockThreads - 1) / kBlockThreads));
    hipStream_t cs;       // behind the segment kernel that produced the partial sums
    if (const int fr = side_stream(h, 1, st.s, &cs)) return fr;
    const ReduceArgs ra = reduce_args(h, st, p);
    if (p.vec4) hipLaunchKernelGGL((spmm_reduce_chunks<4>), rgrid, dim3(kBlockThreads), 0, cs, ra);
    else hipLaunchKernelGGL((spmm_reduce_chunks<1>), rgrid, dim3(kBlockThreads), 0, cs, ra);
    ++*launches;
    return MI_SPMM_OK;
}

// One column part [col0, col0 + N) of the step: the small-step kernel, or the roles' own kernels.  Segment, hub, block and reduce kernels walk
// their whole tables and keep the rows of this call's range; the hub kernel goes first (its longest row is the step's longest dependent chain).
// The first part records the step's diagnostics.
int run_part(mi_spmm_handle *h, const Step &st, int64_t col0, int32_t N, int *launches_out)
{
    Part p;
    int rc = make_part(h, st, col0, N, &p);
    if (rc != MI_SPMM_OK) return rc;
    int launches = 0;
    const bool fused = col0 == 0 && enqueue_small_step(h, st, p, &launches);
    if (!fused) {
        rc = enqueue_hubs(h, st, p, &launches);
        if (rc == MI_SPMM_OK) rc = enqueue_segments(h, st, p, &launches);
        if (rc == MI_SPMM_OK) rc = enqueue_block_passes(h, st, p, &launches);
        if (rc == MI_SPMM_OK) rc = enqueue_rows(h, st, p, &launches);
        if (rc == MI_SPMM_OK) rc = enqueue_reduce(h, st, p, &launches);
        if (rc != MI_SPMM_OK) return rc;
    }
    if (col0 == 0) {
        h->last_fused = fused ? 1 : 0;
        h->last_rows_deep = !fused && rows_deep(h, p) ? 1 : 0;      // (the small-step kernel's rows role is 8 deep)
        h->last_wide = p.wide ? 1 : 0;
        h->last_lpr = p.lpr;
        h->last_v = p.V;
    }
    *launches_out += launches;
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

static int launch_set(mi_spmm_handle *h, const float *d_vin, int64_t ldb, float *d_vout, int64_t ldc, int32_t row_begin,
                      int32_t row_end, const PeerOut &po, hipStream_t s);

int mi_spmm_run_rows(mi_spmm_handle *h, const float *d_vin, int64_t ldb, float *d_vout, int64_t ldc,
                     int32_t row_begin, int32_t row_end, void *stream)
{
    return mi_spmm_run_rows_multi(h, d_vin, ldb, d_vout, ldc, row_begin, row_end, 0, nullptr, stream);
}

int mi_spmm_run_rows_multi(mi_spmm_handle *h, const float *d_vin, int64_t ldb, float *d_vout, int64_t ldc,
                           int32_t row_begin, int32_t row_end, int32_t n_extra, float *const *d_extra, void *stream)
{
    if (!good(h) || !h->prepared) return MI_SPMM_ESTATE;
    if (n_extra < 0 || n_extra > kMaxPeerOut || (n_extra > 0 && !d_extra)) return MI_SPMM_EINVAL;
    PeerOut po;
    std::memset(&po, 0, sizeof(po));
    po.n = n_extra;
    for (int q = 0; q < n_extra; ++q) {
        if (!d_extra[q]) return MI_SPMM_EINVAL;
        po.p[q] = d_extra[q];
    }
    const int32_t M = h->num_v, N = h->feat;
    if (row_begin < 0 || row_end > M || row_begin > row_end) return MI_SPMM_EINVAL;
    if (row_begin == row_end || N == 0) return MI_SPMM_OK;
    if (!d_vout || ldc < N || ldb < N) return MI_SPMM_EINVAL;
    if (!d_vin && h->nnz > 0) return MI_SPMM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    return launch_set(h, d_vin, ldb, d_vout, ldc, row_begin, row_end, po, s);
}

// The launch set of one step (or row panel) on stream s: what run() enqueues, directly or -- once -- under capture.
static int launch_set(mi_spmm_handle *h, const float *d_vin, int64_t ldb, float *d_vout, int64_t ldc, int32_t row_begin,
                      int32_t row_end, const PeerOut &po, hipStream_t s)
{
    const int32_t N = h->feat;
    const int n_extra = po.n;
    float *const *d_extra = po.p;
    bool aligned16 = (N % 4 == 0) && (ldb % 4 == 0) && (ldc % 4 == 0) &&
                     (((uintptr_t)d_vin | (uintptr_t)d_vout) & 15u) == 0;
    for (int q = 0; q < n_extra; ++q) aligned16 = aligned16 && ((uintptr_t)d_extra[q] & 15u) == 0;
    const bool blocks_on = h->n_blk_groups > 0 && aligned16;
    const Step st = {d_vin, d_vout, N, po, ldb, ldc, row_begin, row_end, blocks_on, s};
    // Widths just above a multiple of 256: the last 256-column tile would hold only a few columns yet run one
    // row per wave.  Up to 64 such columns go to a second set of launches with their own, narrower lane groups:
    // N = 257 / 260: -7 % time; wider remainders measured neutral, so they stay tiles of the one launch
    // (profiles/r01_odd_widths.txt -- the partial tile is bound by the extra cache lines, not by instruction issue).
    int32_t rem = (h->split_cols && N > 256) ? N % 256 : 0;
    if (rem > 64) rem = 0;
    int launches = 0;
    h->fork_recorded = h->forked[0] = h->forked[1] = false;
    int rc = run_part(h, st, 0, N - rem, &launches);
    if (rc == 0 && rem > 0) rc = run_part(h, st, N - rem, rem, &launches);
    for (int i = 0; i < 2; ++i) {      // join: whatever the caller enqueues next is ordered after the side streams' rows too
        if (!h->forked[i]) continue;
        h->forked[i] = false;
        hipError_t je = hipEventRecord(h->ev_join[i], h->side[i]);
        if (je == hipSuccess) je = hipStreamWaitEvent(s, h->ev_join[i], 0);
        if (rc == 0 && je != hipSuccess) rc = (int)je;
    }
    h->last_launches = launches;
    return rc;
}


// "autotune": time the step under the plan in force (nothing else: no allocation beyond two events).  One warm-up, then enough runs for ~1 ms.
static int time_step(mi_spmm_handle *h, const float *d_vin, float *d_vout, hipEvent_t e0, hipEvent_t e1, double *ms_out)
{
    PeerOut po;
    std::memset(&po, 0, sizeof(po));
    constexpr double kBytesPerMs = 8e9;      // 8 TB/s
    const double est_ms = gather_bytes(h->nnz, h->num_v, h->feat) / kBytesPerMs;
    int reps = (int)(1.0 / (est_ms > 0.01 ? est_ms : 0.01)) + 1;
    reps = reps < 3 ? 3 : (reps > 20 ? 20 : reps);
    double best = 1e30;
    for (int batch = 0; batch < 2; ++batch) {                  // (min of two batches; the first also warms the plan's tables up)
        int rc = launch_set(h, d_vin, h->feat, d_vout, h->feat, 0, h->num_v, po, nullptr);
        if (rc != MI_SPMM_OK) return rc;
        HIP_TRY(hipEventRecord(e0, nullptr));
        for (int i = 0; i < reps && rc == MI_SPMM_OK; ++i) rc = launch_set(h, d_vin, h->feat, d_vout, h->feat, 0, h->num_v, po, nullptr);
        if (rc != MI_SPMM_OK) return rc;
        HIP_TRY(hipEventRecord(e1, nullptr));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        if ((double)ms / reps < best) best = (double)ms / reps;
    }
    *ms_out = best;
    return MI_SPMM_OK;
}

static int autotune_plan(mi_spmm_handle *h, const float *d_vin, float *d_vout)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return MI_SPMM_ENOMEM; }
    // what the caller left to us (an explicit value of the caller's is never touched); candidates go to in_force, user stays the caller's
    const Tunables &u = h->user;
    const bool own_tile = u.tile_cols == 0, own_strips = u.col_strips == 0, own_mthr = u.medium_thr == 0, own_fused = u.fused_step == 2, own_order = u.seg_order == 0;
    const bool own_unroll = u.rows_unroll == 0, own_thr = u.hub_thr == 0 && !h->split_long && h->feat >= 4;
    Tunables best = h->in_force;        // (= user: the plan in force is the auto plan)
    double best_ms = 0.0;
    int rc = time_step(h, d_vin, d_vout, e0, e1, &best_ms);
    h->tune_auto_ms = best_ms;
    h->tune_evals = 0;
    const int32_t N = h->feat, S_auto = h->n_strips, tile_auto = h->last_lpr * 4, mthr_auto = (int32_t)h->medium_res;
    const bool fused_auto = h->last_fused != 0, rows_deep_auto = h->last_rows_deep != 0;
    const int64_t thr_auto = h->long_thr;        // the resolved hub threshold of the auto plan (1 << 30: the hub fold; 8192 with no row above it: no hubs)
    auto consider = [&](const Tunables &c) {
        if (rc != MI_SPMM_OK) return;
        h->in_force = c;
        rc = preprocess_plan(h);
        double ms = 0.0;
        if (rc == MI_SPMM_OK) rc = time_step(h, d_vin, d_vout, e0, e1, &ms);
        if (rc != MI_SPMM_OK) return;
        ++h->tune_evals;
        if (ms < 0.97 * best_ms) { best = c; best_ms = ms; }    // 3 %: a candidate has to beat the noise of a 1 ms measurement
    };
    // one option at a time, each sweep starting from the best so far (the options interact little once the plan class is fixed: scripts/regret.py)
    // the hub threshold one notch down and one up (a power-of-two ladder, 256 ... 8192): half of auto is 5 - 10 % faster on yelp- / youtube-shaped graphs and an
    // R-MAT of scale 18, 4 - 15 % slower on ddi- / protein-shaped ones and an R-MAT of scale 20 -- no plan statistic separates them (profiles/r05_regret*.md)
    if (own_thr && thr_auto >= 256 && thr_auto <= 8192 && h->max_row_nnz > 256)
        for (int64_t t : {thr_auto / 2, thr_auto * 2}) if (t >= 256 && t <= 8192 && (t < thr_auto || h->max_row_nnz > thr_auto)) { Tunables c = best; c.hub_thr = t; consider(c); }
    if (own_mthr) for (int64_t m : {32, 64, 256, 1024}) if (m != mthr_auto) { Tunables c = best; c.medium_thr = m; consider(c); }
    if (own_strips) {
        const int64_t cand[3] = {1, S_auto > 1 ? (S_auto / 2 > 1 ? S_auto / 2 : 2) : 4, S_auto > 1 ? (2 * S_auto < kMaxColStrips ? 2 * S_auto : kMaxColStrips) : 12};
        for (int64_t sc : cand) if (sc != S_auto) { Tunables c = best; c.col_strips = sc; consider(c); }
    }
    if (own_tile && N > 64) for (int64_t t : {64, 128, 256}) if (t != tile_auto && (t < N || t == 256) && !(t == 256 && tile_auto >= N)) { Tunables c = best; c.tile_cols = t; consider(c); }
    if (own_fused) { Tunables c = best; c.fused_step = fused_auto ? 0 : 1; consider(c); }
    if (own_order && h->n_chunks > 0) { Tunables c = best; c.seg_order = 2; consider(c); }        // segments as the rows come (auto: by length)
    // 16 gathers in flight per lane group of the rows kernel (auto: 8): -13 % on banded 300-700 rows at N = 256, -8 % on rows of 4 - 12 at N = 128 / 256,
    // -1 % on C1 / C2, +4 ... +23 % on community-ordered graphs (occupancy): no rule of the plan's statistics separates them (profiles/r05_rows_unroll_ab.txt)
    if (own_unroll && !fused_auto) { Tunables c = best; c.rows_unroll = rows_deep_auto ? 8 : 16; consider(c); }      // (the other depth than the rule's)
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != MI_SPMM_OK) { h->in_force = h->user; return rc; }
    h->in_force = best;
    h->tune_best_ms = best_ms;
    return preprocess_plan(h);              // the winner's plan (also when the winner is the auto plan: the last candidate's tables are in place otherwise)
}

int mi_spmm_preprocess(mi_spmm_handle *h, const float *d_vin, float *d_vout)
{
    // the reference zeroes vout here (spmm_opt.cu:67-68) because its kernel accumulates; ours overwrites, so vout is left alone -- unless "autotune" is on
    if (good(h)) h->in_force = h->user;     // what an earlier tuning chose goes back to the caller's settings: tuned again below, or simply auto
    const int rc = preprocess_plan(h);
    if (rc != MI_SPMM_OK) return rc;
    if (h->autotune && d_vin && d_vout && h->num_v > 0 && h->feat >= 4 && h->nnz > 0 && !h->split_long) {
        const auto t0 = std::chrono::steady_clock::now();
        const int trc = autotune_plan(h, d_vin, d_vout);
        if (trc != MI_SPMM_OK) return trc;
        h->preprocess_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    return MI_SPMM_OK;
}

int mi_spmm_run_ld(mi_spmm_handle *h, const float *d_vin, int64_t ldb, float *d_vout, int64_t ldc,
                   void *stream)
{
    if (!good(h)) return MI_SPMM_ESTATE;
    return mi_spmm_run_rows(h, d_vin, ldb, d_vout, ldc, 0, h->num_v, stream);
}

int mi_spmm_run(mi_spmm_handle *h, const float *d_vin, float *d_vout, void *stream)
{
    if (!good(h)) return MI_SPMM_ESTATE;
    return mi_spmm_run_rows(h, d_vin, h->feat, d_vout, h->feat, 0, h->num_v, stream);
}

static int compare_common(const void *a, const void *b, int64_t n, int mode, int64_t *count_out,
                          float *maxabs_out, void *stream)
{
    if (!count_out || n < 0) return MI_SPMM_EINVAL;
    *count_out = 0;
    if (maxabs_out) *maxabs_out = 0.f;
    if (n == 0) return MI_SPMM_OK;
    if (!a || !b) return MI_SPMM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *d = nullptr;  // [0] count, [1] max bits
    HIP_TRY(hipMalloc((void **)&d, 256));
    hipError_t e = hipMemsetAsync(d, 0, 16, s);
    if (e == hipSuccess) {
        const int64_t want = (n + kBlockThreads * 4 - 1) / (kBlockThreads * 4);
        const int grid = (int)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
        hipLaunchKernelGGL(compare_kernel, dim3(grid), dim3(kBlockThreads), 0, s, a, b, n, mode, d,
                           (unsigned int *)(d + 1));
        e = hipGetLastError();
    }
    unsigned long long host[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(host, d, 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) return (int)e;
    *count_out = (int64_t)host[0];
    if (maxabs_out) {
        const unsigned int bits = (unsigned int)host[1];
        std::memcpy(maxabs_out, &bits, 4);
    }
    return MI_SPMM_OK;
}

int mi_spmm_valid_float(const float *d_y, const float *d_y2, int64_t n, int64_t *bad_out, void *stream)
{
    return compare_common(d_y, d_y2, n, 0, bad_out, nullptr, stream);
}

int mi_spmm_valid_int(const int32_t *d_y, const int32_t *d_y2, int64_t n, int64_t *bad_out, void *stream)
{
    return compare_common(d_y, d_y2, n, 1, bad_out, nullptr, stream);
}

int mi_spmm_count_bitdiff(const float *d_a, const float *d_b, int64_t n, int64_t *ndiff_out,
                          float *maxabs_out, void *stream)
{
    return compare_common(d_a, d_b, n, 2, ndiff_out, maxabs_out, stream);
}

int mi_spmm_stream_create_concurrent(void **stream_out, int high_priority, int *overlaps_out)
{
    if (!stream_out) return MI_SPMM_EINVAL;
    *stream_out = nullptr;
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));      // hi = numerically lowest = highest priority
    hipStream_t s = nullptr;
    int ov = 0;
    const int rc = concurrent_stream(&s, high_priority ? hi : 0, &ov);
    if (rc != MI_SPMM_OK) return rc;
    *stream_out = (void *)s;
    if (overlaps_out) *overlaps_out = ov;
    return MI_SPMM_OK;
}

int mi_spmm_fill_normal(float *d_out, int64_t n, uint64_t seed, uint64_t subsequence, float mean, float stddev,
                        void *stream)
{
    if (n < 0) return MI_SPMM_EINVAL;
    if (n == 0) return MI_SPMM_OK;
    if (!d_out) return MI_SPMM_EINVAL;
    const int64_t want = ((n + 3) / 4 + kBlockThreads - 1) / kBlockThreads;
    const int grid = (int)(want < 1 ? 1 : (want > 65536 ? 65536 : want));
    hipLaunchKernelGGL(fill_normal_kernel, dim3(grid), dim3(kBlockThreads), 0, (hipStream_t)stream, d_out, n, seed,
                       subsequence, mean, stddev);
    return (int)hipGetLastError();
}

int mi_spmm_fill_philox_u32(uint32_t *d_out, int64_t n, uint64_t seed, uint64_t subsequence, void *stream)
{
    if (n < 0) return MI_SPMM_EINVAL;
    if (n == 0) return MI_SPMM_OK;
    if (!d_out) return MI_SPMM_EINVAL;
    const int64_t want = ((n + 3) / 4 + kBlockThreads - 1) / kBlockThreads;
    const int grid = (int)(want < 1 ? 1 : (want > 65536 ? 65536 : want));
    hipLaunchKernelGGL(fill_philox_kernel, dim3(grid), dim3(kBlockThreads), 0, (hipStream_t)stream, d_out, n, seed,
                       subsequence);
    return (int)hipGetLastError();
}

int mi_spmm_unpack_gathered(const float *d_staging, float *d_C, int64_t rows, int32_t n_ranks,
                            int32_t n_loc, int64_t ldc, void *stream)
{
    if (rows < 0 || n_ranks < 1 || n_loc < 0 || ldc < (int64_t)n_ranks * n_loc) return MI_SPMM_EINVAL;
    if (rows == 0 || n_loc == 0) return MI_SPMM_OK;
    if (!d_staging || !d_C) return MI_SPMM_EINVAL;
    const bool vec4 = (n_loc % 4 == 0) && (ldc % 4 == 0) &&
                      (((uintptr_t)d_staging | (uintptr_t)d_C) & 15u) == 0;
    const int V = vec4 ? 4 : 1;
    const int64_t total = rows * (int64_t)n_ranks * (n_loc / V);
    const int64_t want = (total + kBlockThreads - 1) / kBlockThreads;
    const int grid = (int)(want < 1 ? 1 : (want > 16384 ? 16384 : want));
    hipStream_t s = (hipStream_t)stream;
    if (vec4) hipLaunchKernelGGL((unpack_gathered<4>), dim3(grid), dim3(kBlockThreads), 0, s, d_staging, d_C, rows, n_ranks, n_loc, ldc);
    else hipLaunchKernelGGL((unpack_gathered<1>), dim3(grid), dim3(kBlockThreads), 0, s, d_staging, d_C, rows, n_ranks, n_loc, ldc);
    return (int)hipGetLastError();
}

}  // extern "C"
