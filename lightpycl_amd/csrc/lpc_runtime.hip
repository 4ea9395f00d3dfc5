// lpc_runtime.hip -- host runtime behind the C ABI of include/lpc.h.
//
// One lpc_handle per GPU: a HIP stream, the uploaded scene (filter / exact /
// vertex records + mesh tables), a chunk workspace and the device-resident ray
// population of a trace.  All launches go to the handle's stream.
#include "lpc_kernels.hip"
#include "lpc_emit.hip"
#include "lpc.h"
#include "lpc_comm.hpp"
#include "lpc_build.hpp"
#include "lpc_resource.hpp"
#include <hip/hip_ext.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

using namespace lpck;
using lpcr::DBuf;
using lpcr::Event;
using lpcr::Pinned;
using lpcr::Stream;

static double host_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace {

// 8 SoA arrays (ox oy oz dx dy dz pw | pmid), st floats apart from f, as a RaysIn / RaysOut
template <class R, class F> static R soa_rows(F *f, int64_t st)
{
    R r;
    r.ox = f; r.oy = f + st; r.oz = f + 2 * st; r.dx = f + 3 * st; r.dy = f + 4 * st; r.dz = f + 5 * st;
    r.pw = f + 6 * st; r.pmid = (decltype(r.pmid))(f + 7 * st);
    return r;
}

// ... in one allocation.
struct Pop {
    DBuf buf;
    int64_t cap = 0;
    float *f(int k) const { return (float *)buf.p + (size_t)k * cap; }
    int32_t *pmid() const { return (int32_t *)f(7); }
    RaysIn in(int64_t off = 0) const { return soa_rows<RaysIn>((const float *)f(0) + off, cap); }
    RaysOut out(int64_t off = 0) const { return soa_rows<RaysOut>(f(0) + off, cap); }
};

struct PieceTable {
    DBuf pieces, spieces;              // hierarchy pieces (k_roots_s / k_rootwalk), sliver pieces (k_slivers)
    int32_t npieces = 0, nspieces = 0;
    DBuf groups;                       // k_roots_s gate: the runs' root records, s_lo/s_hi = their pieces
    int32_t ngroups = 0;               // 0: no gate (pieces are the run roots, or > 64 runs)
    std::vector<float> sdmin;          // per sliver piece (ascending): min dmin of its slivers
};

// The trace's current population and its role: the one record of it.  An enqueued
// iteration replaces it whole, a discarded one puts it back (Pending::before).
struct PopState {
    int64_t n = 0;              // rays (iter_collect: the kept children)
    double dmax2 = INFINITY;    // their max |D|^2 (iter_collect)
    bool init = false;          // the population is I (the emitted rays, set_rays), else A
    bool traced = false;        // it is in its parents' traced order
    bool emitted = false;       // it is the emitted rays (set_rays)
    bool pbox_ok = false;       // d_pbox holds its origin box
};

const int kShadeF = 12;   // float arrays of the shade outputs
const int kShadeI = 8;    // int arrays
const int kAccRing = 8;   // mapped counter slots (iterations in flight: at most 2)
const int64_t kCullSlots = 16384;   // iterations the culled-power ledger holds (256 KB on the device)

// Launch policy.  Each value won its A/B (DESIGN.md sections 5 and 7; the losing
// alternatives and their knobs were removed in round 5, the tables there keep the
// record).  None of them changes a result: every path flushes with
// order-independent atomics and the filters are supersets of the exact test.
const int64_t kSortMin = 4096;          // populations below this are traced unsorted
const int64_t kOnesweepMin = 500000;    // rocPRIM onesweep radix sort from this many rays (merge sort below)
const int kRootsPerBlock = 16;          // k_roots_s packets per block (one task per packet)
#ifndef LPC_Q_TARGET
#define LPC_Q_TARGET 65536               // compile-time A/B builds (tools/build_variant.py)
#endif
const int64_t kQTarget = LPC_Q_TARGET;  // (packet, piece) root tests to aim for: the piece level
#ifndef LPC_CHAIN_PIECES
#define LPC_CHAIN_PIECES 4              // compile-time A/B builds (tools/build_variant.py)
#endif
// chained populations up to kChainPiecesMax rays whose target gives the run roots
// (g = 1) in a scene of fewer than kChainPiecesRuns live mesh runs take the pieces
// of g = kChainPieces instead (round 5 A/B, DESIGN.md section 5: lens 10 M -21 %;
// the eye's >= 38 M-ray iterations +1-2 %, hence the size cap; the 10-run
// synthetic scene's config 5 +5 % (dense -3 %), hence the run bound)
const int32_t kChainPieces = LPC_CHAIN_PIECES;
const int64_t kChainPiecesMax = (int64_t)32 << 20;
const int64_t kChainPiecesRuns = 8;
#ifndef LPC_WALK_GRID
#define LPC_WALK_GRID 65536             // compile-time A/B builds (tools/build_variant.py)
#endif
const int64_t kWalkWaves = LPC_WALK_GRID;   // k_rootwalk grid (single-wave blocks, grid-stride)
const int64_t kSliverMergePpw = 4;      // packets per merged sliver unit (k_rootwalk's tail)
const int64_t kSliverWaves = 16384;     // k_slivers: (packet, piece) waves to aim for
#ifndef LPC_SPILL_LEVELS
#define LPC_SPILL_LEVELS 3               // compile-time A/B builds (tools/build_variant.py)
#endif
const int kSpillLevels = LPC_SPILL_LEVELS;  // k_spill levels (hand-over depth) for populations >= kSpillSmallN
const int kSpillLevelsSmall = 1;        // ... below (round 5 A/B: 4 levels, level budgets 10 or 14 / 8, two
                                        //   levels below: neutral or slower)
const int64_t kSpillSmallN = 262144;
#ifndef LPC_SPILL_BLOCKS
#define LPC_SPILL_BLOCKS 4096            // compile-time A/B builds (tools/build_variant.py)
#endif
const int64_t kSpillBlocks = LPC_SPILL_BLOCKS;  // k_spill level l grid: max(kSpillMinBlocks, kSpillBlocks >> l) x 4 waves
const int64_t kSpillMinBlocks = 256;
const int kSpillPairShift = 5;          // exact pairs per node visit in the hand-over budget (log2; round 5
                                        //   A/B with the pair list: 4 and 6 equal)
const int kKeyObits = 6;                // re-sorted populations: origin bits per axis of the 5-D Morton key
const double kThin = 1.0;               // thin-triangle rule factor (thin_axis; 0.25 / 2 measured slower)

}  // namespace

// The timing events of lpc_prof_enable skip the system-scope fence of an event
// record (cache writeback + invalidate: ~7 us of GPU idle per walk launch with
// it, ~0 without; round 5 A/B).  The side stream's fork /
// join events keep it (a device-scope release measured equal).
static const unsigned kEvTimingFlags = hipEventDisableSystemFence;

// The uploaded scene: what lpc_scene_upload and build_records produce.  Usable
// only while `ready`: an upload validates its arguments on locals, then
// scene_invalidate(), the members filled in place (the grow-only buffers are
// kept), scene_publish() last.  An early return in between leaves "no scene".
struct Scene {
    bool ready = false;
    int32_t M = 0, K = 0, Mpad = 0;
    std::vector<float> hv[3];                       // host copies, made on demand from d_raw (rebuilds, profiling)
    DBuf d_raw;                                     // the scene's v0 | v1 | v2 rows on the device ((M,4) each)
    DBuf d_verts, d_mat, d_ior, d_refl, d_diss, d_nodes, d_srec, d_xrec;
    DBuf d_live;                                    // [K] slot written by some run
    std::vector<int32_t> run_lo, run_hi;
    std::vector<std::vector<int32_t>> run_levels;    // per run: (first node, count) per level, root first
    std::vector<FiltRec> node_self;                  // each node's own test (piece roots)
    std::vector<int32_t> run_slo, run_shi;           // sliver records per run
    std::vector<float> sliver_dmin_host;             // SliverRec::dmin, host copy
    int64_t n_slivers = 0, n_thin = 0;               // ... of them thin triangles (thin_axis, k = 1)
    std::vector<int32_t> slot_run, meas_meshes;
    bool mat_passive = false;                       // no material can raise a ray's power (lpc_scene_upload)
    uint32_t refr = 0;                              // refr_mask: the refractive meshes among the first 32
    float box_lo[3] = {0, 0, 0}, box_scale[3] = {1, 1, 1};
    double scene_scale = 1.0, dcap = 16.0;           // half diagonal of the scene box (filter h), the filter's Dcap
    std::map<std::vector<int32_t>, PieceTable> ptabs;   // by the hierarchy level each live run is cut at
    DBuf d_fan;                                     // profiling: fan-triangle flags (SpillArgs::fan)
};

// What set_rays (host rows, device-born sources, a staged batch turning
// current) records about the emitted rays in I; assigned whole (emitted_rays).
struct Emitted {
    bool ready = false;
    int64_t n_init = 0;
    double init_dmax2 = INFINITY;                   // max |D|^2 of the emitted rays
    bool pow_nonneg = false;                        // every emitted power >= 0
    int init_key_lo = 0, init_key_hi = 32;          // key bits that vary over the emitted rays
    bool init_bsort = false;                        // their sort may be the counting sort (bsort_fits)
    float max_ray_len = 1e3f, ior_env = 1.0f;
};

// Size switches and test hooks, read once from the environment in lpc_open;
// only lpc_set_walk_grid and lpc_set_chunk write theirs afterwards.
struct Knobs {
    int half = 3;                                   // LPC_HALF: 3 = half-line cull at the piece roots of chained
                                                    //   populations (run_intersect), 0 = off
    int64_t chunk = 0;                              // LPC_CHUNK: rays per chunk (0 -> default)
    int64_t resort_min = 2000000;                   // LPC_RESORT_MIN: chained traced populations from here re-sort
    int64_t sliver_merge = 0;                       // LPC_SLIVER_MERGE: sliver units in k_rootwalk's grid from a size
                                                    //   (0: always; -1: never, k_slivers on the side stream)
    int64_t walk_grid = kWalkWaves;                 // LPC_WALK_GRID: k_rootwalk blocks
    bool spec = true;                               // LPC_SPEC: speculative iterations (trace_run)
    bool bsort = true;                              // LPC_BSORT: 0 = the emitted rays sort by rocPRIM even where the
                                                    //   counting sort fits (A/B and test hook; the order is the same)
    bool packet_fold = true;                        // LPC_PACKET_FOLD: the merged sliver units' packet bounds as extra
                                                    //   blocks of the k_roots_s launch; 0 = k_packet, a launch of its
                                                    //   own (A/B and test hook; the same PacketRec bits)
    bool roots_lds = true;                          // LPC_ROOTS_LDS: k_roots_s asks for the LDS its batch's records
                                                    //   need; 0 = for a full batch's (A/B hook)
    bool shade_fast = true;                         // LPC_SHADE_FAST: k_shade_stage's single-slot path; 0 = every wave
                                                    //   takes postproc (A/B and test hook; the same bits)
    double dcap_init = 16.0;                        // LPC_DCAP_MILLI / 1000 (tests: a rebuild inside a trace)
    int spill_budget = 20;                          // LPC_BUDGET: node visits before a wave hands its work over (0 off)
    int64_t spill_large_per_tri = 16;               // LPC_LARGE_PER_TRI
    int64_t spill_cap = (int64_t)1 << 22;           // LPC_SPILL_CAP: k_spill queue capacity (items)
    int host_prof = 0;                              // LPC_HOSTPROF: host-side timing of each iteration (stderr);
                                                    //   2: also each launch's hand-over queue lengths (synchronising)
    int map_slices = 6;                             // LPC_MAP_SLICES: k_map_hist keeps the map in LDS while it fits this
                                                    //   many slices (one sweep each); 0 = always global atomics
    int map_per_cu = 8;                             // LPC_MAP_PER_CU: its blocks per CU on the global-atomic paths
};

// What the last launch left in the slot arrays and the launch words.  ensure_ws
// assigns it whole (fresh arrays: nothing is clean), run_intersect takes it by
// value and clears it, enqueue_fused_chunk assigns it whole at its end.
struct SlotState {
    bool clean = false;                             // every slot is (max_ray_len mrl, idx -1, count 0)
    float mrl = 0.0f;
    bool misc_clean = false;                        // the launch words were reset for the next launch
};

// The per 256-tile group counts: two buffers of `cap` words in w_gsum, zero when
// unused.  A traced launch adds into the first ng groups of buffer `par` (word
// offset cur) while its k_stage_move zeroes the dirty_next groups the launch
// before left in the other (offset next); then the buffers swap roles.
struct GroupWords {
    int64_t cap = 0;
    int par = 0;
    int64_t dirty[2] = {0, 0};
    struct Turn { size_t cur, next; int64_t dirty_next; };
    Turn turn(int64_t ng)
    {
        const Turn t{(size_t)par * (size_t)cap, (size_t)(1 - par) * (size_t)cap, dirty[1 - par]};
        dirty[1 - par] = 0; dirty[par] = ng; par = 1 - par;
        return t;
    }
};

// ---- the ledgers of a trace (DESIGN.md section 17 has their life cycle) ------
// A ledger's device memory, with whether it may be non-zero: lpc_trace_reset
// clears what is dirty (ledgers_clear), the handle frees it.  As per-iteration
// rows: kCullSlots of them, allocated once and zeroed, row i for slot i.
struct LedgerBuf {
    DBuf buf;
    bool dirty = false;
    template <class Row> Row *row(int64_t i) const { return (Row *)buf.p + i; }
};
// The trace's table beside two staging tables, [3 tables][cols][n] entries of 8
// bytes: an iteration sums into the staging table of its slot's parity, zeroed
// before its first chunk, and the table joins the trace's only when the
// iteration is collected.
struct StagedTable : LedgerBuf {
    int cols;
    int64_t n = -1;                                 // the entries per column it is laid out for
    explicit StagedTable(int c) : cols(c) {}
    size_t table() const { return (size_t)cols * (size_t)n; }
    double *total() const { return (double *)buf.p; }
    double *staging(int par) const { return total() + (size_t)(1 + par) * table(); }
    double *col(double *t, int c) const { return t + (size_t)c * (size_t)n; }
    bool live() const { return buf.p && n > 0; }
};
// Which ledgers an iteration runs with (the switches as they stood at its enqueue).
struct LedgerSet {
    bool cut = false, bud = false, surf = false, vol = false;
    bool rec() const { return bud || surf || vol; } // the shading's BUD instantiations write the fate records
};
struct Ledgers {
    float min_power = 0.0f;                         // lpc_trace_set_min_power; 0: off (the compaction's default
                                                    //   instantiations)
    bool budget = false;                            // lpc_trace_set_budget; off: the shading's default instantiations
    bool surface = false;                           // lpc_trace_set_surface; off: no seventh fate array
    int64_t it_done = 0;                            // iterations collected since the trace's reset: the next slot
    bool bud_seen = false;                          // an iteration since the reset was enqueued with the budget on
    LedgerBuf cull;                                 // lpc_trace_culled: CullSlot rows
    DBuf w_cull;                                    // per-tile culled counts / powers of one launch
    LedgerBuf bud;                                  // lpc_trace_budget: BudgetRow rows ...
    StagedTable bud_mesh{2};                        // ... and per mesh: power, count of [K][4]
    StagedTable surf{3};                            // lpc_trace_surface: incident, deposited, count of [M]
    bool volume = false;                            // lpc_trace_set_volume; off: no dest in the fate records
    lpc::VolumeGrid vgrid = {};                     // the grid last set (dims 0: never), kept when the map goes off
    int64_t vV = 0;                                 // its voxels
    StagedTable vol{1};                             // lpc_trace_volume: [V + 2], the voxels, outside, segments
    DBuf w_rec;                                     // fate records of one chunk (BudgetRec: 6 arrays of ws_rays, 7
                                                    //   with the surface map on, 10 with the volume map on): a
                                                    //   ledger that reads them on
};

// Every GPU resource of the handle is held by an owner of lpc_resource.hpp and
// goes with it; lpc_close names no member.  The one rule: members are destroyed
// in reverse declaration order, so a stream is declared before everything that
// may be in flight on it -- buffers and events go first, the streams last.
struct lpc_handle {
    int device = 0;
    Stream stream;
    Stream stream2;                                 // side stream: the sliver kernels beside the hierarchy stage
    std::string err;
    char name[256] = {0};
    int cus = 0;
    Knobs knobs;
    Scene scene;
    int64_t scene_gen = 0;                          // scenes invalidated (a staged scan's key box)
    Emitted emitted;                                // the rays in I
    // workspace
    int64_t ws_rays = 0;
    DBuf w_key, w_sc, w_rs, w_shf, w_shi, w_blk_cnt, w_blk_off, w_blk_pow;
    DBuf w_soa, w_stage, w_sort, w_sort_tmp;
    DBuf w_aos;                                     // rays as 32-byte rows for the coherence gather
    DBuf w_tm;                                      // per ray: the slots a flush wrote (traced path, K <= 32)
    DBuf w_bhist;                                   // its per-block hi-digit counts + digit totals
    int64_t m_inflight = 0;                         // populations of the iterations enqueued, not yet read
    DBuf w_fc;                                      // k_shade_stage tile counts / power / max |dir|^2
    DBuf w_gsum;                                    // per 256-tile group counts (GroupWords)
    GroupWords groups;
    SlotState slots;                                // w_key / w_sc / d_misc as the last launch left them
    DBuf w_pk;                                     // PacketRec per 128-ray wave (k_slivers)
    DBuf d_misc;                                    // LPC_MISC_WORDS per-launch words
    size_t sort_tmp_bytes = 0;
    DBuf w_spill;                                   // k_spill queue
    DBuf w_qroots;                                  // root items
    Pinned<DevAcc> acc_host;                        // pinned copy of d_acc (one read per iteration)
    Pinned<DevAcc> acc_map;                         // mapped pinned ring k_scan / k_stage_move publish into
    DevAcc *acc_map_dev = nullptr;                  // (slot seq % kAccRing; + device address)
    // speculative iterations (trace_run, LPC_SPEC): iteration i + 1 is enqueued
    // device-sized (IterCtl) before iteration i's counters are read
    DBuf d_ctl;                                     // IterCtl
    int ctl_par = 0;                                // the parity the next enqueued iteration reads
    std::vector<double> hist_r;                     // the last trace_run's populations / its first (the
    int32_t hist_iter = -1;                         //   speculation's prediction) and its iteration limit
    bool dcap_rebuilt = false;                      // check_dcap rebuilt the records (a speculative iteration is void)
    unsigned int acc_seq = 0;
    bool side_tried = false;                        // stream2 / ev_side created on first use (side_stream)
    // results export (lpc_trace_iterate_export): k_export packs a chunk's part of
    // the results tuple into xst[par] on the main stream, the export stream copies
    // it to the caller's host block while the next kernels run
    struct Export {
        Stream xstream;
        Event ev_xready[2], ev_xdone[2];
        bool xdone_rec[2] = {false, false};         // ev_xdone[par] recorded (the staging may still be read)
        DBuf xst[2];
        int xpar = 0;
        bool x_inflight = false;                    // copies queued on xstream
    } xp;
    Event ev_side[2];                               // rays ready (main -> side), slivers done (side -> main)
    double host_last = 0.0;
    bool mp_valid = false;                          // mp_last = the trace's measured power per measure mesh
    DBuf d_mrun;                                    // its running sums on the device (k_stage_move)
    DBuf d_cbase;                                   // chunked traced iterations: running row bases (ping-pong)
    DBuf w_tbox, d_pbox;                            // per-tile boxes (k_shade_stage), the population's box (k_stage_move)
    double mp_last[LPC_MP_MAX] = {0, 0, 0, 0};
    Ledgers led;                                    // the power cutoff, the power budget, the surface map
    // trace
    Pop A, B, T, I;
    PopState pop;                                   // which of them is current, and as what
    bool inflight = false;                          // the stream may still run a trace's last kernels (settle)
    DBuf m_buf;                                     // measured: x y z pw | mesh
    int64_t m_cap = 0, m_total = 0;
    DBuf d_acc;
    DBuf d_tmp;                                     // misc small device scratch
    DBuf d_scan;                                    // RayScan of set_rays (k_ray_scan)
    DBuf d_mt, d_rng, d_etile;                      // device-born sources: generator state (key | pos), its
                                                    //   doubles, the fixed-order sums' tiles
    // profiling (lpc_prof_enable / lpc_prof_read)
    struct Prof {
        bool on = false, stats = false, light = false;
        std::vector<std::pair<Event, Event>> ev_isect, ev_rest, ev_kern;   // recorded, not yet resolved
        std::vector<Event> ev_pool;
        double isect_ms = 0.0, rest_ms = 0.0, kern_ms = 0.0;
        int64_t launches = 0, pairs = 0;
        int every = 1;                              // light mode: events on every every-th walk launch
        int64_t seq = 0;                            // ... walk launches seen
        DBuf d_stats;                               // walk counters
    } prof;
    // ray-sharded trace (lpc_set_allreduce): the termination decisions and the
    // trace-end aggregates over all ranks
    lpc_allreduce_fn xchg = nullptr;
    void *xchg_ctx = nullptr;
    std::vector<lpc_iter_stats> gstats;             // all-reduced per-iteration stats of the last lpc_trace_run
    double xchg_us = 0.0;                           // host time inside the hook (lpc_prof)
    int64_t xchg_calls = 0;
    // streamed batches of new rays (lpc_trace_stage_rays / lpc_trace_run_staged_async):
    // a FIFO of up to two staged batches, each copied to the device by a helper
    // thread on the copy stream while the handle traces the batch before it
    struct RaySlot {
        Pop P;                                      // the batch as SoA rows (swapped with I when it is traced)
        DBuf aos;                                   // its (n,4) origin / direction rows
        DBuf scan;                                  // k_ray_scan of the batch (device) ...
        Pinned<RayScan> scan_host;                  // ... and its pinned copy
        Event ev;                                   // the batch's copies, unpacks and scan done (cstream)
        std::thread th;
        int rc = 0;
        std::string err;
        int64_t n = 0;
        float max_ray_len = 1e3f, ior_env = 1.0f;
        int64_t scan_gen = -1;                      // the scene generation its scan keyed to (-1: none)
    };
    struct Staged {
        Stream cstream;                             // copy stream of the staged batches
        Event ev_stage;                             // main-stream work before a stage call (cstream waits)
        RaySlot rslot[2];
        int rs_head = 0, rs_count = 0;
        void join()                                 // the helpers use the handle: they end before anything goes
        {
            for (auto &s : rslot)
                if (s.th.joinable()) s.th.join();
        }
        ~Staged() { join(); }
    } stage;
};

static std::string g_open_err;

static int set_err(lpc_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg; else g_open_err = msg;
    return code;
}

#define HIPCHK(h, expr)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return set_err(h, LPC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define RETIF(x)                  \
    do {                          \
        int rc_ = (x);            \
        if (rc_) return rc_;      \
    } while (0)

// Picking a kernel's instantiation from a run-time value: f is a generic lambda,
// called with the value as a compile-time constant (decltype(x)::value).
// with_ku: the shading kernels' register-resident slot count KU (shade_eval), the
// smallest of 4, 8, 12, 16 that holds the scene's K meshes, 0 = slots read from
// memory as postproc needs them (K > 16).
template <class F>
static void with_ku(int K, F &&f)
{
    if (K <= 4) f(std::integral_constant<int, 4>{});
    else if (K <= 8) f(std::integral_constant<int, 8>{});
    else if (K <= 12) f(std::integral_constant<int, 12>{});
    else if (K <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 0>{});
}

template <class F>
static void with_bool(bool b, F &&f)
{
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// Wait for a trace's kernels still queued on the stream: lpc_trace_iterate and
// lpc_trace_run_async return once the iteration counters are published, while
// the rows of the next population still move.  Every entry point that copies
// device data to the host or reuses the caller's buffers calls this first.
static int settle(lpc_handle *h)
{
    if (h && h->inflight) {
        h->inflight = false;
        if (h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (h && h->xp.x_inflight) {                    // results-export copies to the caller's host blocks
        h->xp.x_inflight = false;
        if (h->xp.xstream) HIPCHK(h, hipStreamSynchronize(h->xp.xstream));
    }
    return 0;
}

static int dalloc(lpc_handle *h, DBuf &b, size_t bytes, bool keep = false)
{
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return 0;
    // the stream may still use the old buffer (iterations return before their
    // last kernel ends): let it finish before the buffer goes
    if (b.p && h && h->stream) (void)hipStreamSynchronize(h->stream);
    DBuf nb;
    const hipError_t e = nb.alloc(bytes);
    if (e != hipSuccess)
        return set_err(h, LPC_E_NOMEM, "hipMalloc of " + std::to_string(bytes) + " B: " + hipGetErrorString(e));
    if (keep && b.p && b.bytes) {
        HIPCHK(h, hipMemcpyAsync(nb.p, b.p, b.bytes, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    b = std::move(nb);
    return 0;
}

// A ledger's buffer of at least `bytes`, zeroed whole when fresh is set or it had to be allocated.
static int ledger_shape(lpc_handle *h, LedgerBuf &b, size_t bytes, bool fresh = false)
{
    if (b.buf.p && !fresh) return 0;
    RETIF(dalloc(h, b.buf, bytes));
    HIPCHK(h, hipMemsetAsync(b.buf.p, 0, b.buf.bytes, h->stream));
    return 0;
}

// A staged table laid out for n entries per column (another n: a scene of
// another size, which comes with new rays: the table was cleared).
static int staged_shape(lpc_handle *h, StagedTable &T, int64_t n)
{
    if (T.buf.p && T.n == n) return 0;
    RETIF(ledger_shape(h, T, 3 * (size_t)T.cols * (size_t)n * 8, true));
    T.n = n;
    return 0;
}

static int staged_zero(lpc_handle *h, const StagedTable &T, int par)
{
    if (T.n > 0) HIPCHK(h, hipMemsetAsync(T.staging(par), 0, T.table() * 8, h->stream));
    return 0;
}

// The trace's table to the host, column c into the c-th of dst (NULL: skipped),
// n entries each: zeros when it holds nothing or is laid out for another n.
static int staged_read(lpc_handle *h, const StagedTable &T, int64_t n, std::initializer_list<void *> dst)
{
    for (void *d : dst)
        if (d) memset(d, 0, (size_t)n * 8);
    if (!T.dirty) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    int c = 0;
    for (void *d : dst) {
        if (d && T.live() && T.n == n)
            HIPCHK(h, hipMemcpyAsync(d, T.col(T.total(), c), (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
        ++c;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// lpc_trace_reset: a new trace starts at slot 0 with every ledger zero.
static int ledgers_clear(lpc_handle *h)
{
    Ledgers &G = h->led;
    G.it_done = 0;
    G.bud_seen = false;
    for (LedgerBuf *b : std::initializer_list<LedgerBuf *>{&G.cull, &G.bud, &G.bud_mesh, &G.surf, &G.vol}) {
        if (b->dirty && b->buf.p) HIPCHK(h, hipMemsetAsync(b->buf.p, 0, b->buf.bytes, h->stream));
        b->dirty = false;
    }
    return 0;
}

static int pop_reserve(lpc_handle *h, Pop &P, int64_t n)
{
    if (P.cap >= n && P.buf.p) return 0;
    int64_t cap = std::max<int64_t>(n, 1024);
    if (P.buf.p && h->stream) (void)hipStreamSynchronize(h->stream);   // see dalloc
    P.buf.reset();                      // the old rows are not kept: they go before the new block comes
    P.cap = 0;
    RETIF(dalloc(h, P.buf, (size_t)cap * 8 * 4));
    P.cap = cap;
    return 0;
}

static inline unsigned grid1(int64_t n, int bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// ---------------------------------------------------------------------------
// scene records: lpc_build.hpp builds them on the host (runs on host threads)
static int host_threads();
static void host_parts(int64_t n, int T, const std::function<void(int64_t, int64_t, int)> &fn);
static void host_pool_run(int n, const std::function<void(int)> &fn);

// Host copies of the scene's rows, from the device (a filter-record rebuild or
// the profiling fan flags after lpc_scene_upload returned).
static int host_vertices(lpc_handle *h)
{
    Scene &sc = h->scene;
    for (int k = 0; k < 3; ++k) {
        if (sc.hv[k].size() == 4 * (size_t)sc.M) continue;
        std::vector<float> v(4 * (size_t)sc.M);
        HIPCHK(h, hipMemcpy(v.data(), (const float *)sc.d_raw.p + (size_t)k * 4 * sc.M, (size_t)sc.M * 16,
                            hipMemcpyDeviceToHost));
        sc.hv[k].swap(v);
    }
    return 0;
}

// Per mesh run: an 8-wide sphere hierarchy over its triangles in a top-down
// median-split order, every node's test node_record() of ALL triangles below it
// (so the slack does not compound from level to level); triangles whose sphere
// test is degenerate (slivers) or far wider than the triangle (thin) go to the
// run's line-filter list; triangles that can never be hit are dropped.  Results
// do not depend on the order (ties are resolved by triangle index).
// The scene is not ready from here until the caller publishes it; allocations
// and copies come first, the host tables last.
static int build_records(lpc_handle *h, const float *const *rows = nullptr)
{
    Scene &sc = h->scene;
    sc.ready = false;
    sc.ptabs.clear();       // pieces index the records built here
    if (!rows) RETIF(host_vertices(h));              // a rebuild after the upload: the rows from the device
    SceneBuildIn in;
    in.v0 = rows ? rows[0] : sc.hv[0].data(); in.v1 = rows ? rows[1] : sc.hv[1].data();
    in.v2 = rows ? rows[2] : sc.hv[2].data();
    in.run_lo = sc.run_lo.data(); in.run_hi = sc.run_hi.data(); in.nr = sc.run_lo.size();
    in.dcap = sc.dcap; in.scene_scale = sc.scene_scale; in.thin_k = kThin; in.stack_max = LPC_STACK;
    SceneBuildOut out;
    const double t0 = h->knobs.host_prof ? host_us() : 0.0;
    const std::string err = build_scene_records(in, out, [](int n, const std::function<void(int)> &fn) {
        host_pool_run(n, fn);
    });
    if (!err.empty()) return set_err(h, LPC_E_ARG, err);
    if (h->knobs.host_prof)
        fprintf(stderr, "[lpc host] scene records %.1f us (%zu nodes, %zu slivers, %d threads)\n", host_us() - t0,
                out.nodes.size(), out.slivers.size(), host_threads());
    // spare records so no buffer is empty
    if (out.nodes.empty()) { Node8 z; memset(&z, 0, sizeof(z)); out.nodes.push_back(z); }
    if (out.slivers.empty()) {
        SliverRec ss;
        memset(&ss, 0, sizeof(ss));
        ss.a = NAN; ss.idx = -1; ss.dmin = INFINITY;
        out.slivers.push_back(ss);
    }
    // exact records in leaf order (a leaf's 8 records are 384 contiguous bytes:
    // the walk stages them into LDS with one LDS-DMA load), each with its
    // triangle index; 8 spare records at the end, so the last leaf's load stays
    // inside the buffer (round 6; by triangle index before, A/B neutral)
    // (k_exact_records from the rows on the device and the leaf order)
    const double tb0 = h->knobs.host_prof ? host_us() : 0.0;
    const size_t nx = out.xorder.size();
    RETIF(dalloc(h, sc.d_xrec, (nx + 8) * sizeof(ExactRec)));
    RETIF(dalloc(h, h->d_tmp, std::max<size_t>(nx, 1) * 4));
    if (nx) HIPCHK(h, hipMemcpy(h->d_tmp.p, out.xorder.data(), nx * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemsetAsync((ExactRec *)sc.d_xrec.p + nx, 0, 8 * sizeof(ExactRec), h->stream));
    if (nx) {
        const float4 *raw = (const float4 *)sc.d_raw.p;
        hipLaunchKernelGGL(k_exact_records, dim3(grid1((int64_t)nx)), dim3(256), 0, h->stream, (int64_t)nx,
                           (const int32_t *)h->d_tmp.p, raw, raw + sc.M, raw + 2 * (size_t)sc.M,
                           (ExactRec *)sc.d_xrec.p);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));      // d_tmp is reused
    const double tb1 = h->knobs.host_prof ? host_us() : 0.0;
    RETIF(dalloc(h, sc.d_nodes, out.nodes.size() * sizeof(Node8)));
    RETIF(dalloc(h, sc.d_srec, out.slivers.size() * sizeof(SliverRec)));
    HIPCHK(h, hipMemcpy(sc.d_nodes.p, out.nodes.data(), out.nodes.size() * sizeof(Node8), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(sc.d_srec.p, out.slivers.data(), out.slivers.size() * sizeof(SliverRec),
                        hipMemcpyHostToDevice));
    if (h->knobs.host_prof)
        fprintf(stderr, "[lpc host] records upload: exact records %.1f us, nodes %.1f us\n", tb1 - tb0, host_us() - tb1);
    sc.run_levels.swap(out.run_levels); sc.node_self.swap(out.node_self);
    sc.run_slo.swap(out.run_slo); sc.run_shi.swap(out.run_shi);
    sc.n_slivers = out.n_slivers; sc.n_thin = out.n_thin;
    sc.sliver_dmin_host.clear();
    for (const SliverRec &q : out.slivers) sc.sliver_dmin_host.push_back(q.dmin);
    sc.Mpad = (int32_t)out.nodes.size();
    return 0;
}

// Piece table: hierarchy pieces = subtrees of the runs that own a slot (a run
// whose slot a later run overwrites is skipped, as its results are): all nodes
// of the shallowest level with >= g nodes (g = 1: the run roots; q_level picks
// g for a launch).  Sliver pieces = the runs' slivers in blocks of <= 64 (one
// lane each).
static int piece_table(lpc_handle *h, PieceTable **out, int32_t g)
{
    const size_t nr = h->scene.run_levels.size();
    std::vector<int32_t> run_slot(nr, -1);
    for (int32_t j = 0; j < h->scene.K; ++j)
        if (h->scene.slot_run[(size_t)j] >= 0) run_slot[(size_t)h->scene.slot_run[(size_t)j]] = j;
    // the level each live run is cut at: the shallowest with >= g nodes (many g
    // give the same cut, so a scene builds only a few tables)
    std::vector<int32_t> cut(nr, -1);
    for (size_t r = 0; r < nr; ++r) {
        if (run_slot[r] < 0) continue;
        const std::vector<int32_t> &L = h->scene.run_levels[r];
        size_t lv = 0;
        while (lv + 1 < L.size() / 2 && L[2 * lv + 1] < g) ++lv;
        cut[r] = L.empty() ? -2 : (int32_t)lv;
    }
    auto it = h->scene.ptabs.find(cut);
    if (it != h->scene.ptabs.end()) { *out = &it->second; return 0; }
    std::vector<Piece> pcs, spc, grp;
    std::vector<float> sdm;
    auto piece_at = [&](int32_t root, int32_t slot) {   // a node's own test as a piece
        Piece p;
        memset(&p, 0, sizeof(p));
        const FiltRec &t = h->scene.node_self[(size_t)root];
        p.root = root; p.cx = t.cx; p.cy = t.cy; p.cz = t.cz; p.negB = t.negB; p.negA = t.negA;
        p.slot = slot;
        return p;
    };
    for (size_t r = 0; r < nr; ++r) {
        if (run_slot[r] < 0) continue;
        const std::vector<int32_t> &L = h->scene.run_levels[r];
        if (!L.empty()) {
            const size_t lv = (size_t)cut[r];
            Piece gp = piece_at(L[0], run_slot[r]);     // the run root's own test over the run's pieces
            gp.s_lo = (int32_t)pcs.size();
            gp.s_hi = gp.s_lo + L[2 * lv + 1];
            grp.push_back(gp);
            for (int32_t i = 0; i < L[2 * lv + 1]; ++i) pcs.push_back(piece_at(L[2 * lv] + i, run_slot[r]));
        }
        for (int32_t a = h->scene.run_slo[r]; a < h->scene.run_shi[r]; a += 64) {
            Piece p;
            memset(&p, 0, sizeof(p));
            p.root = -1;
            p.s_lo = a;
            p.s_hi = std::min(a + 64, h->scene.run_shi[r]);
            p.slot = run_slot[r];
            spc.push_back(p);
            sdm.push_back(h->scene.sliver_dmin_host[(size_t)a]);     // the run's slivers ascend in dmin
        }
    }
    if (pcs.size() > 65535 || spc.size() > 65535) return set_err(h, LPC_E_ARG, "too many triangle pieces");
    PieceTable t;                       // cached only once complete
    t.npieces = (int32_t)pcs.size();
    t.nspieces = (int32_t)spc.size();
    {   // sliver pieces in ascending dmin: a launch takes the prefix its rays can reach
        std::vector<size_t> o(spc.size());
        for (size_t i = 0; i < o.size(); ++i) o[i] = i;
        std::stable_sort(o.begin(), o.end(), [&](size_t x, size_t y) { return sdm[x] < sdm[y]; });
        std::vector<Piece> s2;
        for (size_t i : o) { s2.push_back(spc[i]); t.sdmin.push_back(sdm[i]); }
        spc.swap(s2);
    }
    auto put = [&](DBuf &b, const std::vector<Piece> &v) {
        RETIF(dalloc(h, b, v.size() * sizeof(Piece)));
        HIPCHK(h, hipMemcpy(b.p, v.data(), v.size() * sizeof(Piece), hipMemcpyHostToDevice));
        return 0;
    };
    if (!pcs.empty()) RETIF(put(t.pieces, pcs));
    if (!spc.empty()) RETIF(put(t.spieces, spc));
    // the gate pays when the runs are cut below their roots (<= 64 runs: one mask)
    if (grp.size() <= 64 && grp.size() < pcs.size()) {
        RETIF(put(t.groups, grp));
        t.ngroups = (int32_t)grp.size();
    }
    *out = &h->scene.ptabs.emplace(cut, std::move(t)).first->second;
    return 0;
}

// Coherence sort: rocPRIM's default algorithm choice (block merge sort up to
// 1 Mi items, onesweep above) below onesweep_min rays, onesweep from there
// (RaySortOnesweep: 8-bit digit passes; forcing it at every size measured slower,
// 189 vs 131 us per 1 M-ray iteration incl. k_raykey/k_gather).
using RaySortCfg = rocprim::default_config;
using RaySortOnesweep = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                   rocprim::default_config, 0>;

// Rays per chunk.  Default: as many as ~32 GB of per-chunk workspace holds (slots
// 12 B per mesh + ~200 B of coherence copies, shade outputs and sort buffers per
// ray), at most 128 Mi: a chunk is also the unit of the coherence sort, and large
// populations (the eye's grow past 100 M rays) trace up to 1.5x faster in 128 Mi
// chunks than in 8 Mi ones.
static int64_t chunk_rays(const lpc_handle *h)
{
    if (h->knobs.chunk > 0) return h->knobs.chunk;
    const int64_t per_ray = (int64_t)12 * std::max(h->scene.K, 1) + 200;
    const int64_t c = ((int64_t)32 << 30) / per_ray;
    return std::max<int64_t>((int64_t)1 << 20, std::min<int64_t>((int64_t)128 << 20, c));
}

// The largest population a device-sized iteration may hold: below the re-sort
// size (a device-sized iteration keeps its parents' order), one chunk, the
// root-item encoding's packet bound.  k_stage_move sizes the next iteration 0
// (it runs empty) when more children are kept, and the host re-runs it.
static int64_t ds_cap(const lpc_handle *h)
{
    const int64_t cap = std::min<int64_t>({h->knobs.resort_min - 1, chunk_rays(h), (int64_t)LPC_Q_MAX_PACKETS * 64});
    return std::max<int64_t>(0, cap);
}

// Workspace for a chunk of `n` rays.
static int ensure_ws(lpc_handle *h, int64_t n)
{
    if (n <= h->ws_rays) return 0;
    {
        const int64_t C = n;
        RETIF(dalloc(h, h->w_key, (size_t)h->scene.K * C * 8));
        RETIF(dalloc(h, h->w_sc, (size_t)h->scene.K * C * 4));
        RETIF(dalloc(h, h->w_rs, (size_t)8 * C * 4));
        RETIF(dalloc(h, h->w_pk, (size_t)((C + 127) / 128) * sizeof(PacketRec)));
        RETIF(dalloc(h, h->d_misc, LPC_MISC_WORDS * 4));
        RETIF(dalloc(h, h->w_shf, (size_t)kShadeF * C * 4));
        RETIF(dalloc(h, h->w_shi, (size_t)kShadeI * C * 4));
        const int64_t nb = (C + 1023) / 1024;
        RETIF(dalloc(h, h->w_blk_cnt, (size_t)3 * nb * 4));
        RETIF(dalloc(h, h->w_blk_off, (size_t)3 * nb * 8));
        RETIF(dalloc(h, h->w_blk_pow, (size_t)nb * 8));
        RETIF(dalloc(h, h->w_soa, (size_t)8 * C * 4));
        RETIF(dalloc(h, h->w_stage, (size_t)C * 16));
        RETIF(dalloc(h, h->w_aos, (size_t)C * 32));
        RETIF(dalloc(h, h->w_tm, (size_t)C * 4));
        RETIF(dalloc(h, h->w_tbox, (size_t)((C + LPC_ST_TILE - 1) / LPC_ST_TILE + 1) * 6 * 4));
        RETIF(dalloc(h, h->d_pbox, 6 * 4));
        HIPCHK(h, hipMemsetAsync(h->w_tm.p, 0, h->w_tm.bytes, h->stream));
        RETIF(dalloc(h, h->w_sort, (size_t)C * 16));    // keys in/out, values in/out
        RETIF(dalloc(h, h->w_bhist, ((size_t)LPC_BS_ND * ((C + LPC_BS_RPB - 1) / LPC_BS_RPB) + 2 * LPC_BS_ND + 8) * 4));
        size_t tb = 0;
        HIPCHK(h, rocprim::radix_sort_pairs<RaySortCfg>(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                                        (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)C, 0,
                                                        32, h->stream));
        size_t tb1 = 0;
        HIPCHK(h, rocprim::radix_sort_pairs<RaySortOnesweep>(nullptr, tb1, (const uint32_t *)nullptr,
                                                             (uint32_t *)nullptr, (const int32_t *)nullptr,
                                                             (int32_t *)nullptr, (size_t)C, 0, 32, h->stream));
        tb = std::max(tb, tb1);
        RETIF(dalloc(h, h->w_sort_tmp, tb));
        const int64_t nt = (C + LPC_ST_TILE - 1) / LPC_ST_TILE;
        RETIF(dalloc(h, h->w_fc, (size_t)nt * (8 + 4 + 4 + 8 * LPC_MP_MAX) + 64));   // staging tiles' power, counts,
                                                                                      // max |dir|^2, measured power
        GroupWords gw;                                                                // group counts, two launches'
        gw.cap = (nt + LPC_ST_GROUP - 1) / LPC_ST_GROUP + 1;
        RETIF(dalloc(h, h->w_gsum, (size_t)2 * gw.cap * 8));
        HIPCHK(h, hipMemsetAsync(h->w_gsum.p, 0, h->w_gsum.bytes, h->stream));
        h->groups = gw;                                 // all zero: buffer 0 first, nothing dirty
        h->slots = SlotState();                         // fresh slot arrays
        h->sort_tmp_bytes = tb;
        h->ws_rays = C;
    }
    return 0;
}

static ShadeOutPtrs shade_ptrs(lpc_handle *h, bool extra)
{
    const size_t C = (size_t)h->ws_rays;
    float *f = (float *)h->w_shf.p;
    int32_t *i = (int32_t *)h->w_shi.p;
    ShadeOutPtrs o;
    o.destx = f + 0 * C; o.desty = f + 1 * C; o.destz = f + 2 * C; o.pw = f + 3 * C;
    o.rdx = f + 4 * C; o.rdy = f + 5 * C; o.rdz = f + 6 * C; o.rpw = f + 7 * C;
    o.tdx = f + 8 * C; o.tdy = f + 9 * C; o.tdz = f + 10 * C; o.tpw = f + 11 * C;
    o.imid = i + 0 * C; o.meas = i + 1 * C; o.rms = i + 2 * C; o.tms = i + 3 * C;
    if (extra) { o.iidx = i + 4 * C; o.n1 = i + 5 * C; o.n2 = i + 6 * C; o.ent = i + 7 * C; }
    else { o.iidx = o.n1 = o.n2 = o.ent = nullptr; }
    return o;
}

static Event ev_get(lpc_handle *h)
{
    Event e;
    if (!h->prof.ev_pool.empty()) {
        e = std::move(h->prof.ev_pool.back());
        h->prof.ev_pool.pop_back();
    } else {
        (void)e.create(kEvTimingFlags);             // empty on failure
    }
    return e;
}

// Resolve recorded event pairs (after a stream sync).
static void prof_resolve(lpc_handle *h)
{
    // pairs whose end has not happened yet (a speculative iteration still queued)
    // stay for a later call
    auto drain = [&](std::vector<std::pair<Event, Event>> &v, double &acc) {
        size_t keep = 0;
        for (auto &pr : v) {
            if (hipEventQuery(pr.second) == hipErrorNotReady) { v[keep++] = std::move(pr); continue; }
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) acc += ms;
            h->prof.ev_pool.push_back(std::move(pr.first));
            h->prof.ev_pool.push_back(std::move(pr.second));
        }
        v.resize(keep);
    };
    drain(h->prof.ev_isect, h->prof.isect_ms);
    drain(h->prof.ev_kern, h->prof.kern_ms);
    drain(h->prof.ev_rest, h->prof.rest_ms);
}

// Device-sized launch of a population whose size the previous iteration left in
// IterCtl (run_intersect / run_queue / run_spill_levels; NULL: host-sized).
struct DevSize {
    const long long *nd;        // population size (device)
    const unsigned *dm2;        // its max |D|^2 (float bits, device)
    int64_t pred;               // expected size: piece level, budgets, grids
    int64_t bound;              // capacity bound: workspaces, root-item shards
};

// One intersect launch: what all its stages share.  run_intersect builds it once
// (rs / perm once the coherence order is made); the stages take it whole.
struct Launch {
    RaysIn in;                          // the rays where the caller holds them ...
    const float *rs = nullptr;          // ... and their coherence copy (8 arrays of stride n), or NULL
    int64_t n = 0;                      // rays (device-sized: the expected size, which shapes the launches)
    const int32_t *perm = nullptr;      // ray index of a position in the coherence order, or NULL (identity)
    float eps = 0.0f, max_ray_len = 0.0f;
    unsigned long long *skey = nullptr, *stats = nullptr;   // the slot arrays; profiling: the walk counters, or NULL
    int32_t *scnt = nullptr;
    const DevSize *ds = nullptr;
    uint32_t *tmask = nullptr;          // the launch's written-slot masks, or NULL
    bool half = false;                  // the half-line cull at the piece roots
    PieceTable *pt = nullptr;           // the pieces of its root items
    const long long *nd() const { return ds ? ds->nd : nullptr; }
};

// Work hand-over (k_spill levels): queue, budget by population size.
static int spill_setup(lpc_handle *h, const Launch &L, SpillArgs *SP)
{
    *SP = SpillArgs{nullptr, nullptr, 0u, 0, 31, L.tmask, nullptr};
    if (h->prof.stats) {                // diagnostic: the fan triangles (apex valence >= 32), built once
        if (!h->scene.d_fan.p) {
            RETIF(host_vertices(h));
            std::map<std::array<uint32_t, 3>, int32_t> val;
            auto key = [&](const std::vector<float> &v, int32_t i) {
                std::array<uint32_t, 3> k;
                memcpy(k.data(), &v[4 * (size_t)i], 12);
                return k;
            };
            const std::vector<float> *hv = h->scene.hv;
            const int32_t M = h->scene.M;
            for (int32_t i = 0; i < M; ++i) { ++val[key(hv[0], i)]; ++val[key(hv[1], i)]; ++val[key(hv[2], i)]; }
            std::vector<uint8_t> f((size_t)M, 0);
            for (int32_t i = 0; i < M; ++i)
                f[(size_t)i] = val[key(hv[0], i)] >= 32 || val[key(hv[1], i)] >= 32 || val[key(hv[2], i)] >= 32;
            RETIF(dalloc(h, h->scene.d_fan, (size_t)h->scene.M));
            HIPCHK(h, hipMemcpy(h->scene.d_fan.p, f.data(), (size_t)h->scene.M, hipMemcpyHostToDevice));
        }
        SP->fan = (const uint8_t *)h->scene.d_fan.p;
    }
    if (h->knobs.spill_budget <= 0) return 0;
    RETIF(dalloc(h, h->w_spill, (size_t)2 * h->knobs.spill_cap * sizeof(SpillItem)));
    SP->items = (SpillItem *)h->w_spill.p;
    SP->ctr = (uint32_t *)h->d_misc.p + LPC_MISC_SPILL;
    SP->cap = (uint32_t)std::min<int64_t>(h->knobs.spill_cap, 0x7fffffff);
    // no hand-over once a population fills the chip many times over (from
    // LPC_LARGE_PER_TRI rays per triangle)
    SP->budget = L.n >= h->knobs.spill_large_per_tri * (int64_t)h->scene.M ? 0 : h->knobs.spill_budget;
    SP->pair_shift = kSpillPairShift;
    return 0;
}

// The rays of a launch as one base of 8 equally spaced arrays (RayBase): the
// coherence copy (stride n) or a population / staging buffer (stride = its
// capacity).  Every RaysIn the runtime builds has this shape.
static int ray_base(lpc_handle *h, const Launch &L, RayBase *out)
{
    if (L.rs) { *out = RayBase{L.rs, L.n}; return 0; }
    const RaysIn &in = L.in;
    const int64_t st = in.oy - in.ox;
    if (in.oz - in.oy != st || in.dx - in.oz != st || in.dy - in.dx != st || in.dz - in.dy != st)
        return set_err(h, LPC_E_ARG, "internal: ray arrays not equally spaced");
    *out = RayBase{in.ox, st};
    return 0;
}

// hand-over levels of a launch of n rays (0: none)
static int spill_level_count(const lpc_handle *h, int64_t n, const SpillArgs &SP)
{
    const int lv = n >= kSpillSmallN ? kSpillLevels : kSpillLevelsSmall;
    return SP.budget > 0 ? std::max(1, std::min(lv, 7)) : 0;
}

// level l's input (queue l % 2, length misc[6 + l]) and output (level l + 1)
static void spill_level_args(lpc_handle *h, const SpillArgs &SP, int l, int levels, SpillArgs *I, SpillArgs *O)
{
    uint32_t *misc = (uint32_t *)h->d_misc.p;
    *I = SP; *O = SP;
    I->items = (SpillItem *)h->w_spill.p + (size_t)(l % 2) * (size_t)h->knobs.spill_cap;
    I->ctr = misc + LPC_MISC_SPILL + l;
    O->items = (SpillItem *)h->w_spill.p + (size_t)((l + 1) % 2) * (size_t)h->knobs.spill_cap;
    O->ctr = misc + LPC_MISC_SPILL + l + 1;
    O->budget = l + 1 < levels ? SP.budget : 0;
}

// hand-over levels: level l reads queue l % 2 (length misc[6 + l]) and queues
// what exceeds the budget for level l + 1; the last level finishes
static int run_spill_levels(lpc_handle *h, const Launch &L, const SpillArgs &SP)
{
    RayBase ray;
    RETIF(ray_base(h, L, &ray));
    const int levels = spill_level_count(h, L.n, SP);
    for (int l = 0; l < levels; ++l) {
        SpillArgs I, O;
        spill_level_args(h, SP, l, levels, &I, &O);
        // later levels hold fewer items (and often none): smaller grids, in
        // 4-wave units, launched as single-wave blocks
        const unsigned g = (unsigned)std::max<int64_t>(kSpillMinBlocks, kSpillBlocks >> l) * 4u;
        // profiling counters only in the PROF instantiation (fewer live registers without)
        with_bool(L.stats != nullptr, [&](auto pf) {
            hipLaunchKernelGGL((k_spill<8, decltype(pf)::value>), dim3(g), dim3(64), 0, h->stream, ray, L.n, L.perm,
                               (const Node8 *)h->scene.d_nodes.p, (const ExactRec *)h->scene.d_xrec.p, L.eps,
                               L.max_ray_len, L.skey, L.scnt, L.stats, I, O, L.nd());
        });
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Piece level of the work queue: pieces per run so that (packets x pieces) root
// tests reach q_target (mesh run roots for large populations, finer pieces for
// small ones, whose few packets would otherwise be few items).
static int32_t q_level(const lpc_handle *h, int64_t n, bool chained)
{
    int64_t live_runs = 0;
    for (int32_t j = 0; j < h->scene.K; ++j) live_runs += h->scene.slot_run[(size_t)j] >= 0;
    live_runs = std::max<int64_t>(live_runs, 1);
    const int64_t npk = (n + 63) / 64;
    const int32_t g = (int32_t)std::min<int64_t>(4096, std::max<int64_t>(1, (kQTarget + npk * live_runs - 1) /
                                                                               (npk * live_runs)));
    return (g == 1 && chained && n <= kChainPiecesMax && live_runs < kChainPiecesRuns) ? kChainPieces : g;
}

// A device-side consistency check failed (QueueArgs::err / the compaction's
// prefix check, kept in DevAcc::qerr): the launch's results are incomplete.
// Clear the flag and report.  Never expected; the checks keep a sizing error from
// silently losing intersections.
static int q_failed(lpc_handle *h)
{
    (void)hipStreamSynchronize(h->stream);
    (void)hipMemset((char *)h->d_acc.p + offsetof(DevAcc, qerr), 0, sizeof(uint32_t));
    return set_err(h, LPC_E_HIP, "device-side consistency check failed (root-item capacity or compaction prefix): "
                                 "results incomplete");
}

static int check_qerr(lpc_handle *h)
{
    uint32_t e = 0;
    HIPCHK(h, hipMemcpy(&e, (char *)h->d_acc.p + offsetof(DevAcc, qerr), sizeof(e), hipMemcpyDeviceToHost));
    return e ? q_failed(h) : 0;
}

// The root-item queue of a launch of n rays: shard capacity, buffer, arguments.
// k_roots_s holds at most 64 LPC_ROOTS_TASKS pieces in LDS: a table with more
// (more than 1 024 live mesh runs, cut at their roots, no gate) is tested in
// batches of that many pieces, one k_roots_s launch each, into the same queue.
#define LPC_ROOTS_BATCH (64 * LPC_ROOTS_TASKS)
struct RootsBatch {
    int S, pb;
    int64_t blocks, vblocks;
};
static RootsBatch roots_batch(int64_t npk, const DevSize *ds, int32_t npieces)
{
    RootsBatch b;
    b.S = (int)((npieces + 63) / 64);           // S tasks per packet (npieces <= 64 S)
    b.pb = b.S >= 3 ? 1 : b.S == 2 ? 2 : kRootsPerBlock;   // pb packets per block
    b.blocks = (npk + b.pb - 1) / b.pb;
    b.vblocks = !ds ? b.blocks : (((ds->bound + 63) / 64) + b.pb - 1) / b.pb;
    return b;
}
struct QueueShape {
    int64_t npk, rs_blocks;
    int rs_S, rs_pb;
    int nbatch;                                 // k_roots_s launches (pieces in batches of LPC_ROOTS_BATCH)
};
static int queue_args(lpc_handle *h, const Launch &L, QueueArgs *Qo, QueueShape *sh)
{
    const PieceTable *pt = L.pt;
    const DevSize *ds = L.ds;
    // device-sized (ds): n is the expected size (grids), the bound sizes the shards
    const int64_t npk = (L.n + 63) / 64;
    const int nbatch = std::max(1, (int)((pt->npieces + LPC_ROOTS_BATCH - 1) / LPC_ROOTS_BATCH));
    if (nbatch > 1 && pt->ngroups > 0) return set_err(h, LPC_E_STATE, "internal: gated pieces in several batches");
    const RootsBatch b0 = roots_batch(npk, ds, std::min<int32_t>(pt->npieces, LPC_ROOTS_BATCH));
    // per shard: at most its blocks' packets x pieces items, summed over the batches
    // (k_roots_s / k_gather_roots flag an overflow through Q.err instead of dropping
    // items silently)
    int64_t rcap = 0;
    for (int k = 0; k < nbatch; ++k) {
        const int32_t np = std::min<int32_t>(pt->npieces - k * LPC_ROOTS_BATCH, LPC_ROOTS_BATCH);
        const RootsBatch b = roots_batch(npk, ds, np);
        rcap += ((b.vblocks + LPC_Q_CSHARDS - 1) / LPC_Q_CSHARDS) * b.pb * (int64_t)np;
    }
    // k_gather_roots: one packet per wave of its blocks
    const int64_t gpb = LPC_GR_T / 64;
    rcap = std::max<int64_t>(rcap, ((((npk + gpb - 1) / gpb) + LPC_Q_CSHARDS - 1) / LPC_Q_CSHARDS) * gpb *
                                       (int64_t)pt->npieces);
    if (rcap >= 0xffffffffLL) return set_err(h, LPC_E_ARG, "root items: too many per shard");
    RETIF(dalloc(h, h->w_qroots, (size_t)LPC_Q_CSHARDS * (size_t)rcap * 8));
    *Qo = QueueArgs{(uint64_t *)h->w_qroots.p, (uint32_t *)h->d_misc.p,
                    (uint32_t *)((char *)h->d_acc.p + offsetof(DevAcc, qerr)), (uint32_t)rcap};
    *sh = QueueShape{npk, b0.blocks, b0.S, b0.pb, nbatch};
    return 0;
}

// The hierarchy stage: k_roots_s writes the (packet, piece) items whose root test
// passes, k_rootwalk walks them grid-stride and hands heavy subtrees to the
// k_spill levels.  merged: the sliver units of the walk's
// tail, or NULL.  roots_done: k_gather_roots already wrote the items (same queue
// arguments).  *sampled: the walk launch carries profiling events.
static int run_queue(lpc_handle *h, const Launch &L, const SliverArgs *merged, bool roots_done, bool *sampled)
{
    const int64_t n = L.n;
    const PieceTable *pt = L.pt;
    QueueArgs Q;
    QueueShape sh;
    RETIF(queue_args(h, L, &Q, &sh));
    if (h->knobs.host_prof)
        fprintf(stderr, "[lpc host] roots: n %lld packets %lld pieces %d groups %d S %d pb %d blocks %lld rcap %lld\n",
                (long long)n, (long long)sh.npk, (int)pt->npieces, (int)pt->ngroups, sh.rs_S, sh.rs_pb,
                (long long)sh.rs_blocks, (long long)Q.rcap);
    // merged sliver tests (LPC_SLIVER_MERGE): the packet bounds before the walk,
    // on this stream; the walk's waves take the (packet group, piece) units.
    // The bounds are ceil(npkx / 4) more blocks of the first k_roots_s launch
    // (LPC_PACKET_FOLD); k_packet where there is none (k_gather_roots wrote the
    // items: folded in there it was slower) or the knob is off
    const int64_t npkx = (n + 127) / 128;
    const bool fold = merged && !roots_done && h->knobs.packet_fold;
    for (int k = 0; !roots_done && k < sh.nbatch; ++k) {
        const int32_t np = std::min<int32_t>(pt->npieces - k * LPC_ROOTS_BATCH, LPC_ROOTS_BATCH);
        const RootsBatch b = roots_batch(sh.npk, L.ds, np);
        const Piece *pc = (const Piece *)pt->pieces.p + (size_t)k * LPC_ROOTS_BATCH;
        const int64_t rblocks = std::max<int64_t>(b.blocks, 1);
        const int64_t pblocks = (fold && k == 0) ? (npkx + 3) / 4 : 0;
        const dim3 rg((unsigned)(rblocks + pblocks));
        // the records' LDS: 20 B per piece and group of this batch
        const size_t lds = (size_t)20 * (h->knobs.roots_lds ? (size_t)np + (size_t)pt->ngroups
                                                             : (size_t)LPC_ROOTS_BATCH + 64);
        with_bool(L.half, [&](auto hf) {
            hipLaunchKernelGGL(k_roots_s<decltype(hf)::value>, rg, dim3(256), lds, h->stream, L.in, L.rs, n, pc, (int)np,
                               (const Piece *)pt->groups.p, (int)pt->ngroups, Q, b.S, b.pb, L.nd(),
                               pblocks ? (PacketRec *)h->w_pk.p : nullptr, (int)rblocks);
        });
    }
    SliverArgs SA;
    memset(&SA, 0, sizeof(SA));
    if (merged) {
        SA = *merged;
        if (!fold)
            hipLaunchKernelGGL(k_packet<2>, dim3((unsigned)((npkx + 3) / 4)), dim3(256), 0, h->stream, L.in, L.rs, n,
                               (PacketRec *)h->w_pk.p, L.nd());
    }
    RayBase ray;
    RETIF(ray_base(h, L, &ray));
    SpillArgs SP;
    RETIF(spill_setup(h, L, &SP));
    const unsigned grid = (unsigned)h->knobs.walk_grid;      // single-wave blocks
    // profiling: the launch's own start/stop timestamps (hipExtLaunchKernel), no
    // event packets between the kernels
    Event k0, k1;
    // light mode samples every prof_every-th launch: a launch with events costs
    // ~7 us more (bench A/B)
    *sampled = h->prof.on && (!h->prof.light || h->prof.seq++ % h->prof.every == 0);
    if (*sampled) { k0 = ev_get(h); k1 = ev_get(h); }
    // profiling counters only in the PROF instantiation, the merged sliver units
    // only in the MERGED one (fewer live registers without: the plain walk holds
    // 7 waves per SIMD, the merged one 6)
    with_bool(L.stats != nullptr, [&](auto pf) {
        with_bool(merged != nullptr, [&](auto mg) {
            hipExtLaunchKernelGGL((k_rootwalk<8, decltype(pf)::value, decltype(mg)::value>), dim3(grid), dim3(64), 0,
                                  h->stream, k0, k1, 0, ray, n, L.perm, (const Node8 *)h->scene.d_nodes.p,
                                  (const ExactRec *)h->scene.d_xrec.p, L.eps, L.max_ray_len, L.skey, L.scnt, L.stats,
                                  Q, SP, L.nd(), SA);
        });
    });
    if (*sampled) h->prof.ev_kern.emplace_back(std::move(k0), std::move(k1));
    RETIF(run_spill_levels(h, L, SP));
    if (h->knobs.host_prof >= 2) {                          // diagnostic: this launch's hand-over queue lengths
        uint32_t q[8] = {0};
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(q, (uint32_t *)h->d_misc.p + LPC_MISC_SPILL, sizeof(q), hipMemcpyDeviceToHost));
        fprintf(stderr, "[lpc host] hand-over: n %lld items per level %u %u %u %u\n", (long long)n, q[0], q[1], q[2],
                q[3]);
    }
    return 0;
}

// the side stream of the sliver kernels and its fork / join events, created on
// first use (a handle whose slivers run in the walk's grid holds one stream, so
// several handles in flight each keep a hardware queue of their own); false:
// all on the main stream
static bool side_stream(lpc_handle *h)
{
    if (!h->side_tried) {
        h->side_tried = true;
        if (h->stream2.create() != hipSuccess || h->ev_side[0].create() != hipSuccess ||
            h->ev_side[1].create() != hipSuccess) {
            (void)hipGetLastError();
            h->stream2.reset();
            for (Event &e : h->ev_side) e.reset();
        }
    }
    return h->stream2 && h->ev_side[0] && h->ev_side[1];
}

// One intersect launch's inputs and outputs (run_intersect).  The drop-in calls
// leave trace / traced / ds / acc_reset at their defaults: no cull, no masks,
// the iteration counters untouched.
struct IsectIn {
    RaysIn rays;
    int64_t n = 0;
    float max_ray_len = 0.0f;
    double dmax2 = INFINITY;                        // max |D|^2 of the rays (sliver pieces in reach)
    float *st_user = nullptr;                       // optional: the caller's [ray][mesh] distances,
    int32_t *si_user = nullptr, *sc_user = nullptr; //   triangle indices, counts
    const DevSize *ds = nullptr;
    bool trace = false;                             // an iteration of the trace, over its population ...
    bool traced = false;                            // ... without per-ray exports
    bool acc_reset = false;                         // the launch's slot reset also resets the iteration counters,
    int64_t acc_total = 0;                          //   to this measured total (iter_enqueue, a one-chunk iteration)
};
struct IsectOut {
    RaysIn traced;                                  // IsectIn::traced: the rays in the launch's order
    uint32_t *tmask = nullptr;                      // this launch's written-slot masks (k_shade_stage reads them)
    bool sampled = false;                           // the walk launch carries profiling events
};

// ---- the other stages of one intersect launch, in launch order (run_intersect) ----
// The piece cut: q_level's (the same sliver pieces at every cut), coarser while
// k_roots_s cannot hold the pieces (tiny populations; a table of more than 1 024
// run roots, g = 1, goes to k_roots_s in batches).
static int piece_cut(lpc_handle *h, int64_t n, bool chained, PieceTable **pt)
{
    int32_t g = q_level(h, n, chained);
    RETIF(piece_table(h, pt, g));
    while ((*pt)->npieces > LPC_ROOTS_BATCH && g > 1) {
        g = std::max(1, g / 8);
        RETIF(piece_table(h, pt, g));
    }
    return 0;
}

// The slot / launch-word reset; returns the SlotInit the key kernel is to carry.
// Traced iterations (k_shade_stage) leave every slot they read in the clean state
// (max_ray_len, idx -1, count 0) and k_stage_move resets the launch words for the
// next launch, so a traced launch after one (`was`) resets less; where the key
// kernel runs before everything that reads the launch words (fold), it carries the
// reset.  "counters": the iteration counters too, where a.acc_reset asks (with
// clean slots never: k_stage_move writes every counter).
//   traced  slots clean  fold  words clean | k_slot_init launched here           | the key kernel carries
//   yes     no           -     -           | whole array, masks, words, counters | -
//   yes     yes          yes   -           | -                                   | words
//   yes     yes          no    no          | words                               | -
//   yes     yes          no    yes         | -                                   | -
//   no      -            yes   -           | -                                   | n rays' slots, words, counters
//   no      -            no    -           | n rays' slots, words, counters      | -
static SlotInit slot_reset(lpc_handle *h, const Launch &L, const IsectIn &a, bool fold, SlotState was)
{
    SlotInit SI;
    SI.K = h->scene.K; SI.live = (const int32_t *)h->scene.d_live.p; SI.max_ray_len = L.max_ray_len;
    SI.skey = L.skey; SI.scnt = L.scnt; SI.misc = (uint32_t *)h->d_misc.p;
    SI.acc = a.acc_reset ? (DevAcc *)h->d_acc.p : nullptr;
    SI.m_total = (unsigned long long)a.acc_total;
    SI.uniform = 0; SI.tmask = nullptr;
    SlotInit none = SI;
    none.skey = nullptr; none.misc = nullptr; none.acc = nullptr;
    auto launch = [&](int64_t rays) {
        hipLaunchKernelGGL(k_slot_init, dim3(grid1(std::max<int64_t>(rays, LPC_MISC_WORDS))), dim3(256), 0, h->stream,
                           rays, SI);
    };
    const bool clean = a.traced && was.clean && was.mrl == L.max_ray_len;
    if (a.traced && !clean) {           // the whole array to the clean state (stride-independent)
        SI.uniform = 1;
        SI.tmask = (uint32_t *)h->w_tm.p;
        launch(h->ws_rays);
        return none;
    }
    if (clean) { SI.skey = nullptr; SI.acc = nullptr; }     // the launch words only
    if (fold) return SI;
    if (!(clean && was.misc_clean)) launch(clean ? 0 : L.n);
    return none;
}

// The coherence order of a launch of at least kSortMin rays: rays of one wave
// share origin cell and direction (key [scene-box origin cell | direction]),
// sorted by the counting sort or rocPRIM, then gathered from the 32-byte rows the
// key kernel wrote -- with the root tests fused in (k_gather_roots) when the
// launch has one root-test task per packet and no run gate (roots_done: it wrote
// the root items).  SIk: slot_reset's.
struct Order { const float *rs = nullptr; const int32_t *perm = nullptr; bool roots_done = false; };
static int coherence_order(lpc_handle *h, const Launch &L, const IsectIn &a, const SlotInit &SIk, Order *out)
{
    const RaysIn &in = L.in;
    const int64_t n = L.n;
    const bool traced = a.traced;
    const float *blo = h->scene.box_lo, *bsc = h->scene.box_scale;     // the coherence key's box
    const size_t C = (size_t)h->ws_rays;
    uint32_t *kin = (uint32_t *)h->w_sort.p, *kout = kin + C;
    int32_t *vin = (int32_t *)(kout + C), *vout = vin + C;
    // the emitted rays' varying key bits (set_rays)
    int b0 = 0, b1 = 32;
    if (traced && h->pop.emitted) { b0 = h->emitted.init_key_lo; b1 = h->emitted.init_key_hi; }
    const int nbits = b1 - b0;
    if (traced && h->pop.emitted && h->emitted.init_bsort && h->knobs.bsort && nbits >= 1 && nbits <= 16 &&
        n >= LPC_MISC_WORDS) {
        // counting sort (MSD, two 8-bit digits, stable), then the gather
        const int hb = std::min(nbits, LPC_BS_HB), lb = nbits - hb;
        const int64_t nblk = (n + LPC_BS_RPB - 1) / LPC_BS_RPB;
        uint32_t *hist = (uint32_t *)h->w_bhist.p, *tot = hist + (size_t)LPC_BS_ND * nblk;
        uint32_t *bst = tot + LPC_BS_ND;
        hipLaunchKernelGGL(k_bkey, dim3((unsigned)nblk), dim3(LPC_BS_T), 0, h->stream, in, n, blo[0], blo[1],
                           blo[2], bsc[0], bsc[1], bsc[2], kin, (float4 *)h->w_aos.p, SIk, b0, lb, hb, hist, nblk);
        hipLaunchKernelGGL(k_bprefix, dim3(1u << hb), dim3(256), 0, h->stream, hist, nblk, tot);
        hipLaunchKernelGGL(k_bscatter, dim3((unsigned)nblk), dim3(LPC_BS_T), 0, h->stream, (const uint32_t *)kin,
                           n, b0, lb, hb, (const uint32_t *)hist, nblk, (const uint32_t *)tot, bst,
                           (uint8_t *)kout, vin, vout);
        if (lb > 0)
            hipLaunchKernelGGL(k_bsort2, dim3(1u << hb, LPC_BS_MAXB / LPC_BS_RPB), dim3(LPC_BS_T), 0, h->stream,
                               (const uint8_t *)kout, (const int32_t *)vin, lb, (const uint32_t *)bst, vout);
    } else {
        // a re-sorted chained population: the key (5-D Morton) spans its own box
        // (k_stage_move of the iteration that made it), not the scene's
        const uint32_t *pbox = (traced && h->pop.traced && h->pop.pbox_ok) ? (const uint32_t *)h->d_pbox.p : nullptr;
        hipLaunchKernelGGL(k_raykey, dim3(grid1(n)), dim3(256), 0, h->stream, in, n, blo[0], blo[1], blo[2], bsc[0],
                           bsc[1], bsc[2], kin, vin, (float4 *)h->w_aos.p, SIk, pbox, pbox ? kKeyObits : 5,
                           pbox ? 1 : 0);
        size_t tb = h->sort_tmp_bytes;
        if (n >= kOnesweepMin)          // large populations: onesweep (one pass per 8 key bits)
            HIPCHK(h, rocprim::radix_sort_pairs<RaySortOnesweep>(h->w_sort_tmp.p, tb, kin, kout, vin, vout,
                                                                 (size_t)n, b0, b1, h->stream));
        else
            HIPCHK(h, rocprim::radix_sort_pairs<RaySortCfg>(h->w_sort_tmp.p, tb, kin, kout, vin, vout, (size_t)n,
                                                            b0, b1, h->stream));
    }
    out->perm = vout;
    if (!L.ds && L.pt->npieces > 0 && L.pt->npieces <= 64 && L.pt->ngroups == 0) {
        QueueArgs Qf;
        QueueShape shf;
        RETIF(queue_args(h, L, &Qf, &shf));
        const dim3 gg((unsigned)((n + LPC_GR_T - 1) / LPC_GR_T));
        with_bool(L.half, [&](auto hf) {
            hipLaunchKernelGGL(k_gather_roots<decltype(hf)::value>, gg, dim3(LPC_GR_T), 0, h->stream,
                               (const float4 *)h->w_aos.p, n, out->perm, (float *)h->w_rs.p, traced ? 1 : 0,
                               (const Piece *)L.pt->pieces.p, (int)L.pt->npieces, Qf);
        });
        out->roots_done = true;
    } else {
        hipLaunchKernelGGL(k_gather_aos, dim3(grid1(n)), dim3(256), 0, h->stream, (const float4 *)h->w_aos.p, n,
                           out->perm, (float *)h->w_rs.p, traced ? 1 : 0);
    }
    out->rs = (const float *)h->w_rs.p;
    return 0;
}

// Where a launch's sliver tests run, and over which sliver pieces.
//   merged (LPC_SLIVER_MERGE: from this population size, default every size):
//     as units of the walk's own grid (k_rootwalk's tail), on the main stream;
//   side: k_slivers beside the hierarchy stage on the side stream (both only add
//     to the slots with order-independent atomics), launched after the hierarchy
//     stage's kernels (the host reaches k_roots_s / k_rootwalk sooner), forked
//     before the walk and joined after it.  One stream per trace keeps several
//     traces in flight from interleaving fork / join events;
//   neither: k_slivers before the walk on the main stream (no side stream).
struct SliverPlan {
    int32_t nsp = 0;                    // sliver pieces the rays can reach: dmin <= max |D| (sliver_dmin);
    float dmax = 0.0f;                  //   device-sized: every piece in the grid, culled there by DevSize::dm2
    bool merged = false, side = false;
};
static SliverPlan sliver_plan(lpc_handle *h, const Launch &L, double dmax2)
{
    SliverPlan S;
    if (!(dmax2 >= 0.0)) dmax2 = INFINITY;      // NaN bound (a NaN direction): no culling
    S.dmax = (float)std::min<double>(sqrt(dmax2 * (1.0 + 1e-5)), (double)INFINITY);
    while (S.nsp < L.pt->nspieces && (L.ds || L.pt->sdmin[(size_t)S.nsp] <= S.dmax)) ++S.nsp;
    S.merged = h->knobs.sliver_merge >= 0 && L.n >= h->knobs.sliver_merge && S.nsp > 0 && L.pt->npieces > 0;
    S.side = !S.merged && S.nsp > 0 && side_stream(h);
    return S;
}

// k_slivers' arguments (ppw packets per wave), or the merged units' (run_queue)
static SliverArgs sliver_args(lpc_handle *h, const Launch &L, const SliverPlan &S, int64_t ppw)
{
    SliverArgs A;
    memset(&A, 0, sizeof(A));
    A.R = L.in; A.rs = L.rs; A.n = L.n; A.perm = L.perm; A.pk = (const PacketRec *)h->w_pk.p;
    A.srec = (const SliverRec *)h->scene.d_srec.p; A.pieces = (const Piece *)L.pt->spieces.p; A.nsp = S.nsp;
    A.ppw = (int)ppw; A.eps = L.eps; A.max_ray_len = L.max_ray_len; A.dmax = S.dmax;
    A.skey = L.skey; A.scnt = L.scnt; A.stats = L.stats; A.nd = L.nd(); A.dm2d = L.ds ? L.ds->dm2 : nullptr;
    A.tmask = L.tmask;
    return A;
}

// The unmerged sliver tests: the packet bounds and k_slivers, on the side stream
// between its fork and join events, or on the main stream.
static int launch_slivers(lpc_handle *h, const Launch &L, const SliverPlan &S)
{
    const hipStream_t ss = S.side ? h->stream2 : h->stream;
    if (S.side) HIPCHK(h, hipStreamWaitEvent(h->stream2, h->ev_side[0], 0));
    if (S.nsp > 0) {
        // packets per wave: enough (packet, piece) waves to fill the GPU, no more
        const int64_t npkx = (L.n + 127) / 128;
        const int64_t ppw = std::max<int64_t>(1, npkx * S.nsp / kSliverWaves);
        const dim3 sg((unsigned)((npkx + 4 * ppw - 1) / (4 * ppw)), (unsigned)S.nsp);
        hipLaunchKernelGGL(k_packet<2>, dim3((unsigned)((npkx + 3) / 4)), dim3(256), 0, ss, L.in, L.rs, L.n,
                           (PacketRec *)h->w_pk.p, L.nd());
        hipLaunchKernelGGL(k_slivers, sg, dim3(256), 0, ss, sliver_args(h, L, S, ppw));
        HIPCHK(h, hipGetLastError());
    }
    if (S.side) HIPCHK(h, hipEventRecord(h->ev_side[1], h->stream2));
    return 0;
}

// intersect for a.n rays of a.rays into the slot arrays, and optionally into a
// caller's [ray][mesh] buffers (st_user != NULL, the reference's scratch layout).
// a.traced (trace iterations without per-ray exports): the launch works in
// its coherence order and out->traced receives the rays in that order.
// a.ds != NULL (a speculative trace iteration, chained traced population): n is
// the bound, the kernels read the population size on the device and the
// launch shapes follow ds->pred.
static int run_intersect(lpc_handle *h, const IsectIn &a, IsectOut *out)
{
    *out = IsectOut();
    RETIF(ensure_ws(h, a.n));
    if ((a.n + 63) / 64 > (int64_t)LPC_Q_MAX_PACKETS)
        return set_err(h, LPC_E_STATE, "internal: chunk above the root items' packet bound");
    const bool chained = a.traced && h->pop.traced;   // children in their parents' traced order: no sort of their own
    Launch L;
    L.in = a.rays; L.ds = a.ds;
    L.n = a.ds ? std::max<int64_t>(1, std::min(a.ds->pred, a.n)) : a.n;    // launch shapes
    L.max_ray_len = a.max_ray_len; L.eps = 0.000001f * a.max_ray_len;       // .cl:245, single-precision constant
    L.skey = (unsigned long long *)h->w_key.p; L.scnt = (int32_t *)h->w_sc.p;
    L.stats = h->prof.stats ? (unsigned long long *)h->prof.d_stats.p : nullptr;
    // written-slot masks: kept by every flush of this launch, read by its
    // k_shade_stage (traced launches only; a mask bit may be stale, never missing:
    // the masks are cleared with the slots, and only the traced path reads them)
    L.tmask = out->tmask = (a.traced && h->scene.K <= 32) ? (uint32_t *)h->w_tm.p : nullptr;
    // LPC_HALF 3 (default): the half-line cull at the piece roots (k_roots_s items)
    // of a trace's chained populations; "emitted" = the trace's first population,
    // whatever the export mode; the drop-in kernels (lpc_intersect,
    // lpc_bounce_host: no trace population) are never culled.  0: off.
    L.half = a.trace && h->knobs.half == 3 && !h->pop.emitted;
    RETIF(piece_cut(h, L.n, chained, &L.pt));
    // a chained population keeps its parents' order, except a large one
    // (LPC_RESORT_MIN): after many generations that order has lost its coherence
    const bool sorted = L.n >= kSortMin && (!chained || (!a.ds && L.n >= h->knobs.resort_min));
    const SlotState was = h->slots;
    h->slots = SlotState();
    const SlotInit SIk = slot_reset(h, L, a, /*fold*/ sorted && L.n >= LPC_MISC_WORDS, was);
    Order ord;
    if (sorted) RETIF(coherence_order(h, L, a, SIk, &ord));
    L.rs = ord.rs;
    L.perm = ord.perm;
    if (a.traced) {                     // positions of the coherence order are the rays' indices from here on
        out->traced = L.rs ? soa_rows<RaysIn>(L.rs, L.n) : L.in;
        L.perm = nullptr;
    }
    const SliverPlan S = sliver_plan(h, L, a.dmax2);
    if (S.side) HIPCHK(h, hipEventRecord(h->ev_side[0], h->stream));     // fork
    if (!S.side && !S.merged) RETIF(launch_slivers(h, L, S));
    Event e0, e1;
    if (h->prof.on && !h->prof.light) { e0 = ev_get(h); e1 = ev_get(h); (void)hipEventRecord(e0, h->stream); }
    if (L.pt->npieces > 0) {
        const SliverArgs SAm = sliver_args(h, L, S, kSliverMergePpw);
        RETIF(run_queue(h, L, S.merged ? &SAm : nullptr, ord.roots_done, &out->sampled));
    }
    if (h->prof.on) {      // the intersect stage: the walk (+ k_packet, k_slivers)
        if (!h->prof.light) {
            (void)hipEventRecord(e1, h->stream);
            h->prof.ev_isect.emplace_back(std::move(e0), std::move(e1));
        }
        if (!h->prof.light || out->sampled) {
            h->prof.launches += 1;
            h->prof.pairs += L.n * (int64_t)h->scene.M;
        }
    }
    if (S.side) {
        RETIF(launch_slivers(h, L, S));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_side[1], 0));     // join
    }
    if (a.st_user) {
        hipLaunchKernelGGL(k_slot_export, dim3(grid1(L.n)), dim3(256), 0, h->stream, L.n, h->scene.K,
                           (const int32_t *)h->scene.d_live.p, (const unsigned long long *)L.skey,
                           (const int32_t *)L.scnt, a.st_user, a.si_user, a.sc_user, 1);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

static ShadeArgs shade_args(lpc_handle *h, const RaysIn &in, const int32_t *meas_in, int64_t n, float max_ray_len,
                            float ior_env, bool extra)
{
    ShadeArgs A;
    A.in = in; A.meas_in = meas_in; A.n = n; A.K = h->scene.K;
    A.skey = (const unsigned long long *)h->w_key.p; A.sc = (const int32_t *)h->w_sc.p;
    A.mat_type = (const int32_t *)h->scene.d_mat.p; A.ior = (const float *)h->scene.d_ior.p;
    A.refl = (const float *)h->scene.d_refl.p; A.diss = (const float *)h->scene.d_diss.p;
    A.verts = (const float *)h->scene.d_verts.p;
    A.max_ray_len = max_ray_len; A.ior_env = ior_env;
    A.o = shade_ptrs(h, extra);
    return A;
}

static int run_shade(lpc_handle *h, const RaysIn &in, const int32_t *meas_in, int64_t n,
                     float max_ray_len, float ior_env, bool extra)
{
    const ShadeArgs A = shade_args(h, in, meas_in, n, max_ray_len, ior_env, extra);
    with_ku(h->scene.K, [&](auto ku) {
        hipLaunchKernelGGL(k_shade<decltype(ku)::value>, dim3(grid1(n)), dim3(256), 0, h->stream, A);
    });
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The gates: of every entry point that computes on the scene, and of those that
// trace the emitted rays (they go with their scene).
static int need_scene(lpc_handle *h) { return h->scene.ready ? 0 : set_err(h, LPC_E_STATE, "no scene uploaded"); }
static int need_rays(lpc_handle *h, const char *who)
{
    RETIF(need_scene(h));
    return h->emitted.ready ? 0 : set_err(h, LPC_E_STATE, std::string(who) + " before trace_set_rays");
}

// The old scene goes: what depends on it is marked in this one place.  The
// buffers stay (dalloc grows only); scene_publish ends the filling.
static void scene_invalidate(lpc_handle *h)
{
    h->scene.ready = false;
    h->scene.ptabs.clear();
    h->scene.d_fan.reset();             // profiling flags of the previous scene
    h->emitted = Emitted{};
    h->ws_rays = 0;                     // K may change
    ++h->scene_gen;                     // staged batches' scans keyed to the old box are redone when traced
}
static int scene_publish(lpc_handle *h) { h->scene.ready = true; return 0; }   // the only place

// If |D| of any upcoming ray exceeds the filter's Dcap, rebuild the filter
// records without the tiny-triangle culling (Dcap = inf).  A trace may be running:
// the rebuilt scene keeps its rays and workspace, a failed rebuild leaves neither.
static int check_dcap(lpc_handle *h, double dmax2)
{
    if (dmax2 <= h->scene.dcap * h->scene.dcap * (1.0 - 1e-6)) return 0;
    h->scene.dcap = INFINITY;
    h->dcap_rebuilt = true;
    if (const int rc = build_records(h)) { scene_invalidate(h); return rc; }
    return scene_publish(h);
}

extern "C" {

int lpc_abi_version(void) { return LPC_ABI_VERSION; }

int lpc_device_count(int *count)
{
    if (!count) return set_err(nullptr, LPC_E_ARG, "count is NULL");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return 0;
}

int lpc_device_query(int device, char *name, int name_len, char *arch, int arch_len, int *cu_count)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c)
        return set_err(nullptr, LPC_E_ARG, "no HIP device " + std::to_string(device));
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return set_err(nullptr, LPC_E_HIP, "hipGetDeviceProperties");
    if (name && name_len > 0) { strncpy(name, p.name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    if (arch && arch_len > 0) { strncpy(arch, p.gcnArchName, (size_t)arch_len - 1); arch[arch_len - 1] = 0; }
    if (cu_count) *cu_count = p.multiProcessorCount;
    return 0;
}

int lpc_open(int device, lpc_handle **out)
{
    if (!out) return set_err(nullptr, LPC_E_ARG, "out is NULL");
    *out = nullptr;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c == 0)
        return set_err(nullptr, LPC_E_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device < 0 || device >= c)
        return set_err(nullptr, LPC_E_ARG, "device ordinal " + std::to_string(device) + " out of range");
    struct Closer { void operator()(lpc_handle *p) const { (void)lpc_close(p); } };
    std::unique_ptr<lpc_handle, Closer> owner(new lpc_handle());    // closed on every failure below
    lpc_handle *h = owner.get();
    auto fail = [&](int rc) { g_open_err = h->err; return rc; };  // the handle's message outlives it
    h->device = device;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = h->stream.create();
    if (e != hipSuccess) return set_err(nullptr, LPC_E_HIP, std::string("stream: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        snprintf(h->name, sizeof(h->name), "%s (%s)", prop.name, prop.gcnArchName);
        h->cus = prop.multiProcessorCount;
    }
    int rc = dalloc(h, h->d_acc, sizeof(DevAcc));
    if (!rc) rc = dalloc(h, h->d_mrun, LPC_MP_MAX * sizeof(double));
    if (!rc) rc = dalloc(h, h->d_ctl, sizeof(IterCtl));
    if (rc) return fail(rc);
    if (hipMemset(h->d_acc.p, 0, sizeof(DevAcc)) != hipSuccess ||   // counters start empty (qerr 0)
        hipMemset(h->d_ctl.p, 0, sizeof(IterCtl)) != hipSuccess)
        return set_err(nullptr, LPC_E_HIP, "counter init");
    // results do not depend on the knobs: the tests drive the re-sort, the merged sliver
    // units, the hand-over and its queue overflow, chunked iterations and a records rebuild in a trace at small sizes
    auto env_int = [](const char *k, int64_t dflt) -> int64_t {
        const char *v = getenv(k);
        return (v && *v) ? strtoll(v, nullptr, 10) : dflt;
    };
    Knobs &k = h->knobs;
    k.half = env_int("LPC_HALF", k.half) == 0 ? 0 : 3;
    k.chunk = std::max<int64_t>(0, env_int("LPC_CHUNK", k.chunk));
    k.resort_min = std::max<int64_t>(1, env_int("LPC_RESORT_MIN", k.resort_min));
    k.sliver_merge = env_int("LPC_SLIVER_MERGE", k.sliver_merge);
    k.walk_grid = std::min<int64_t>(std::max<int64_t>(env_int("LPC_WALK_GRID", k.walk_grid), 64), 1 << 22);
    k.spec = env_int("LPC_SPEC", k.spec) != 0;
    k.bsort = env_int("LPC_BSORT", k.bsort) != 0;
    k.packet_fold = env_int("LPC_PACKET_FOLD", k.packet_fold) != 0;
    k.roots_lds = env_int("LPC_ROOTS_LDS", k.roots_lds) != 0;
    k.shade_fast = env_int("LPC_SHADE_FAST", k.shade_fast) != 0;
    k.dcap_init = (double)env_int("LPC_DCAP_MILLI", 16000) / 1000.0;
    k.spill_budget = (int)env_int("LPC_BUDGET", k.spill_budget);
    k.spill_large_per_tri = env_int("LPC_LARGE_PER_TRI", k.spill_large_per_tri);
    k.spill_cap = std::max<int64_t>(env_int("LPC_SPILL_CAP", k.spill_cap), 64);
    k.host_prof = (int)env_int("LPC_HOSTPROF", 0);
    k.map_slices = (int)std::min<int64_t>(1024, std::max<int64_t>(0, env_int("LPC_MAP_SLICES", k.map_slices)));
    k.map_per_cu = (int)std::min<int64_t>(64, std::max<int64_t>(1, env_int("LPC_MAP_PER_CU", k.map_per_cu)));
    if (h->acc_map.alloc(kAccRing * sizeof(DevAcc), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void **)&h->acc_map_dev, h->acc_map, 0) != hipSuccess) {
        h->acc_map.reset();                          // counters then come by copy + stream sync
        h->acc_map_dev = nullptr;
    } else {
        memset(h->acc_map, 0, kAccRing * sizeof(DevAcc));
    }
    if (h->acc_host.alloc(sizeof(DevAcc)) != hipSuccess) return set_err(nullptr, LPC_E_HIP, "pinned host buffer");
    *out = owner.release();
    return 0;
}

int lpc_close(lpc_handle *h)
{
    if (!h) return 0;
    (void)settle(h);                     // a trace still running (lpc_trace_iterate / _run_async)
    (void)hipSetDevice(h->device);
    h->stage.join();
    // nothing is in flight when the members go (their owners release them, in
    // reverse declaration order: see lpc_handle)
    const hipStream_t streams[] = {h->stream, h->stream2, h->xp.xstream, h->stage.cstream};
    for (hipStream_t s : streams)
        if (s) (void)hipStreamSynchronize(s);
    delete h;
    return 0;
}

int lpc_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes)
{
    if (device_bytes) *device_bytes = lpcr::g_device_bytes.load(std::memory_order_relaxed);
    if (pinned_bytes) *pinned_bytes = lpcr::g_pinned_bytes.load(std::memory_order_relaxed);
    return 0;
}

const char *lpc_last_error(const lpc_handle *h) { return h ? h->err.c_str() : g_open_err.c_str(); }

int lpc_device_info(lpc_handle *h, char *name, int name_len, int *cu_count)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (name && name_len > 0) { strncpy(name, h->name, (size_t)name_len - 1); name[name_len - 1] = 0; }
    if (cu_count) *cu_count = h->cus;
    return 0;
}

int lpc_scene_upload(lpc_handle *h, int32_t tri_count, const float *v0, const float *v1,
                     const float *v2, const int32_t *mesh_id, int32_t mesh_count,
                     const int32_t *mat_type, const float *ior, const float *refl,
                     const float *diss)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    // validation, on locals: a refused upload leaves the handle as it was
    if (tri_count <= 0 || mesh_count <= 0 || !v0 || !v1 || !v2 || !mesh_id || !mat_type || !ior || !refl || !diss)
        return set_err(h, LPC_E_ARG, "scene needs >= 1 triangle, >= 1 mesh and all tables");
    // the walk's sparse exact-test pairs hold a triangle index in 26 bits (and root
    // items node ids in 28, LPC_Q_MAX_NODES)
    if (tri_count >= (1 << 26)) return set_err(h, LPC_E_ARG, "scene has too many triangles (limit 2^26 - 1)");
    // the root items carry a mesh's scratch slot in 12 bits (q_item)
    if (mesh_count > LPC_Q_MAX_SLOTS + 1)
        return set_err(h, LPC_E_ARG, "scene has too many meshes (limit " + std::to_string(LPC_Q_MAX_SLOTS + 1) + ")");
    const double tu0 = h->knobs.host_prof ? host_us() : 0.0;
    const int32_t M = tri_count, K = mesh_count;
    for (int32_t i = 0; i < M; ++i)
        if (mesh_id[i] < 0 || mesh_id[i] >= K)
            return set_err(h, LPC_E_ARG, "mesh_id[" + std::to_string(i) + "] out of range");
    // runs of equal mesh_id and the slot each one flushes into (.cl:260-265, 286)
    std::vector<int32_t> run_lo, run_hi, slot_run((size_t)K, -1);
    for (int32_t i = 0; i < M; ++i) {
        if (i == 0 || mesh_id[i] != mesh_id[i - 1]) { run_lo.push_back(i); run_hi.push_back(i + 1); }
        else run_hi.back() = i + 1;
    }
    for (size_t r = 0, nr = run_lo.size(); r < nr; ++r) {
        int32_t slot = (r + 1 < nr) ? mesh_id[run_lo[r + 1]] - 1 : mesh_id[run_lo[r]];
        if (slot < 0)
            return set_err(h, LPC_E_ARG, "mesh_id sequence writes below slot 0 (reference would "
                                         "corrupt another ray's scratch); mesh ids must not decrease to 0");
        slot_run[slot] = (int32_t)r;      // a later run overwrites, as the sequential loop does
    }
    // the old scene goes; until scene_publish below there is none
    scene_invalidate(h);
    Scene &sc = h->scene;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sc.M = M; sc.K = K; sc.dcap = h->knobs.dcap_init;
    sc.run_lo.swap(run_lo); sc.run_hi.swap(run_hi); sc.slot_run.swap(slot_run);
    // the rows go to the device as they are (the vertex and exact records are
    // built there); the host reads the caller's arrays during this call and keeps
    // no copy (host_vertices fetches one for a later rebuild)
    for (auto &v : sc.hv) v.clear();
    RETIF(dalloc(h, sc.d_raw, (size_t)M * 48));
    for (int k = 0; k < 3; ++k)
        HIPCHK(h, hipMemcpyAsync((float *)sc.d_raw.p + (size_t)k * 4 * M, k == 0 ? v0 : k == 1 ? v1 : v2,
                                 (size_t)M * 16, hipMemcpyHostToDevice, h->stream));
    std::vector<int32_t> live((size_t)K);
    for (int32_t j = 0; j < K; ++j) live[(size_t)j] = sc.slot_run[(size_t)j] >= 0;
    RETIF(dalloc(h, sc.d_live, (size_t)K * 4));
    HIPCHK(h, hipMemcpy(sc.d_live.p, live.data(), (size_t)K * 4, hipMemcpyHostToDevice));
    sc.meas_meshes.clear();
    for (int32_t j = 0; j < K; ++j) if (mat_type[j] == 3) sc.meas_meshes.push_back(j);
    sc.refr = lpc::refr_mask(K, mat_type);
    // passive materials: the children of a ray never carry more power than it
    // (refractive: R, T = 1 - R in [0, 1] for finite positive indices,
    // .cl:313-326; mirror: P R with 0 <= R <= 1, .cl:443 -- a negative R flips the
    // sign, so a population's summed power could grow; dissipation only
    // attenuates, .cl:385-394)
    sc.mat_passive = true;
    for (int32_t j = 0; j < K; ++j) {
        if ((mat_type[j] == 0 || mat_type[j] == 4) && !(ior[j] > 0.0f && std::isfinite(ior[j])))
            sc.mat_passive = false;
        if (mat_type[j] == 1 && !(refl[j] >= 0.0f && refl[j] <= 1.0f)) sc.mat_passive = false;
    }
    // vertices (the hit triangle's normal in the shading), from the rows on the device
    RETIF(dalloc(h, sc.d_verts, (size_t)M * 36));
    const float4 *raw = (const float4 *)sc.d_raw.p;
    hipLaunchKernelGGL(k_vertex_rows, dim3(grid1(M)), dim3(256), 0, h->stream, (int64_t)M, raw, raw + M,
                       raw + 2 * (size_t)M, (float *)sc.d_verts.p);
    HIPCHK(h, hipGetLastError());
    {   // scene box for the ray coherence key
        float lo3[3] = {INFINITY, INFINITY, INFINITY}, hi3[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (const float *vs : {v0, v1, v2})
            for (int32_t i = 0; i < M; ++i)
                for (int k = 0; k < 3; ++k) {
                    const float v = vs[4 * (size_t)i + k];
                    if (std::isfinite(v)) { lo3[k] = std::min(lo3[k], v); hi3[k] = std::max(hi3[k], v); }
                }
        double diag2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            const float ext = hi3[k] - lo3[k];
            sc.box_lo[k] = std::isfinite(lo3[k]) ? lo3[k] : 0.0f;
            sc.box_scale[k] = (std::isfinite(ext) && ext > 0.0f) ? 32.0f / ext : 1.0f;
            if (std::isfinite(ext)) diag2 += (double)ext * ext;
        }
        sc.scene_scale = diag2 > 0.0 ? 0.5 * sqrt(diag2) : 1.0;
    }
    const double tu1 = h->knobs.host_prof ? host_us() : 0.0;
    const float *const rows[3] = {v0, v1, v2};
    RETIF(build_records(h, rows));
    const double tu2 = h->knobs.host_prof ? host_us() : 0.0;
    const std::pair<DBuf *, const void *> tabs[] = {{&sc.d_mat, mat_type}, {&sc.d_ior, ior}, {&sc.d_refl, refl},
                                                    {&sc.d_diss, diss}};
    for (const auto &t : tabs) RETIF(dalloc(h, *t.first, (size_t)K * 4));
    for (const auto &t : tabs) HIPCHK(h, hipMemcpy(t.first->p, t.second, (size_t)K * 4, hipMemcpyHostToDevice));
    if (h->knobs.host_prof)
        fprintf(stderr, "[lpc host] scene upload: tables %.1f us, records %.1f us, device copies %.1f us\n", tu1 - tu0,
                tu2 - tu1, host_us() - tu2);
    return scene_publish(h);
}

// The process's host worker threads (host_threads() - 1 of them beside the
// caller), created at first use and kept: a thread start costs tens of us on
// the GPU boxes, which a scene upload or a ray pass would otherwise pay per call.
// One caller at a time; a concurrent caller (a staging helper thread) runs its
// tasks itself.
namespace {
class HostPool {
public:
    explicit HostPool(int workers)
    {
        for (int k = 0; k < workers; ++k) th_.emplace_back([this]() { loop(); });
    }
    ~HostPool()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cv_.notify_all();
        for (std::thread &t : th_) t.join();
    }
    void run(int n, const std::function<void(int)> &fn)
    {
        std::unique_lock<std::mutex> busy(call_, std::try_to_lock);
        if (!busy.owns_lock() || th_.empty() || n <= 1) {
            for (int i = 0; i < n; ++i) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &fn;
            n_ = n;
            next_.store(0);
            active_ = (int)th_.size();
            ++gen_;
        }
        cv_.notify_all();
        for (int i; (i = next_.fetch_add(1)) < n;) fn(i);
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this]() { return active_ == 0; });
        job_ = nullptr;
    }

private:
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *job;
            int n;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                job = job_;
                n = n_;
            }
            for (int i; (i = next_.fetch_add(1)) < n;) (*job)(i);
            std::lock_guard<std::mutex> lk(m_);
            if (--active_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_, call_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *job_ = nullptr;
    int n_ = 0, active_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
    std::atomic<int> next_{0};
};
}  // namespace

static void host_pool_run(int n, const std::function<void(int)> &fn)
{
    static HostPool pool(std::max(0, host_threads() - 1));
    pool.run(n, fn);
}

// Host passes over the caller's rays (set_rays, bounce_host) split over threads:
// fn(lo, hi, part) for T contiguous parts, results combined by the caller in
// part order (so every combine is deterministic).
static void host_parts(int64_t n, int T, const std::function<void(int64_t, int64_t, int)> &fn)
{
    if (T <= 1 || n < (1 << 16)) { fn(0, n, 0); return; }
    host_pool_run(T, [&](int t) { fn(n * t / T, n * (t + 1) / T, t); });
}

static int host_threads()
{
    static int t = [] {
        const char *v = getenv("LPC_HOST_THREADS");
        int k = v && *v ? atoi(v) : (int)std::thread::hardware_concurrency();
        return std::max(1, std::min(k, 16));
    }();
    return t;
}

static double host_dmax2(int64_t n, const float *dir4)
{
    const int T = host_threads();
    std::vector<double> part((size_t)T, 0.0);
    host_parts(n, T, [&](int64_t lo, int64_t hi, int t) {
        double m = 0.0;
        for (int64_t i = lo; i < hi; ++i) {
            const float *d = dir4 + 4 * i;
            double q = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
            if (!(q <= m)) m = q;   // NaN propagates as "large"
        }
        part[(size_t)t] = m;
    });
    double m = 0.0;
    for (double q : part)
        if (!(q <= m)) m = q;
    return m;
}

// (n,4) origin and direction rows on the device into the six SoA arrays that
// start at dst, `st` floats apart (a population: Pop::f(0) + first row, its
// capacity), on stream s.
static void unpack_rays(hipStream_t s, int64_t n, const float4 *o4, const float4 *d4, float *dst, size_t st)
{
    hipLaunchKernelGGL(k_unpack4, dim3(grid1(n)), dim3(256), 0, s, n, o4, dst, dst + st, dst + 2 * st);
    hipLaunchKernelGGL(k_unpack4, dim3(grid1(n)), dim3(256), 0, s, n, d4, dst + 3 * st, dst + 4 * st, dst + 5 * st);
}

// Upload (n,4) host rows into SoA arrays of a population (rows 0..n): both row
// arrays into one staging buffer (the copies return once the host arrays are
// read), then the unpacks on the stream; `sync`: wait for them (the caller may
// reuse the staging buffer at once otherwise).
static int upload_rays(lpc_handle *h, Pop &P, int64_t n, const float *origin4, const float *dir4,
                       const float *pow, const int32_t *prev_mid, bool sync = true)
{
    RETIF(dalloc(h, h->w_stage, (size_t)n * 32));
    float4 *so = (float4 *)h->w_stage.p, *sd = so + n;
    HIPCHK(h, hipMemcpy(so, origin4, (size_t)n * 16, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(sd, dir4, (size_t)n * 16, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(P.f(6), pow, (size_t)n * 4, hipMemcpyHostToDevice));
    unpack_rays(h->stream, n, so, sd, P.f(0), (size_t)P.cap);
    if (prev_mid) HIPCHK(h, hipMemcpy(P.pmid(), prev_mid, (size_t)n * 4, hipMemcpyHostToDevice));
    else                                        // just emitted (-2, iterative_tracer.py:118), filled on the device
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)P.pmid(), -2, (size_t)n, h->stream));
    HIPCHK(h, hipGetLastError());
    if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int lpc_bounce_host(lpc_handle *h, int64_t n, const float *origin4, const float *dir4,
                    float *pow, int32_t *meas, const int32_t *prev_mid, float max_ray_len,
                    float ior_env, float *dest4, int32_t *isect_mid, float *r_dir4, float *r_pow,
                    int32_t *r_meas, float *t_dir4, float *t_pow, int32_t *t_meas,
                    int32_t *n1_mid, int32_t *n2_mid, int32_t *entering, int32_t *isect_idx)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (n < 0 || !origin4 || !dir4 || !pow || !meas || !prev_mid || !dest4 || !isect_mid ||
        !r_dir4 || !r_pow || !r_meas || !t_dir4 || !t_pow || !t_meas)
        return set_err(h, LPC_E_ARG, "bounce_host: missing buffer");
    if (n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    const double bdmax2 = host_dmax2(n, dir4);
    RETIF(check_dcap(h, bdmax2));
    const int64_t C = std::min(n, chunk_rays(h));
    RETIF(ensure_ws(h, C));
    Pop P;
    RETIF(pop_reserve(h, P, C));
    DBuf dmeas;
    RETIF(dalloc(h, dmeas, (size_t)C * 4));
    int rc = 0;
    for (int64_t base = 0; base < n && !rc; base += C) {
        const int64_t nc = std::min(C, n - base);
        rc = upload_rays(h, P, nc, origin4 + 4 * base, dir4 + 4 * base, pow + base, prev_mid + base);
        if (rc) break;
        if (hipMemcpy(dmeas.p, meas + base, (size_t)nc * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = set_err(h, LPC_E_HIP, "meas upload"); break; }
        IsectOut io;
        rc = run_intersect(h, IsectIn{P.in(), nc, max_ray_len, bdmax2}, &io);
        if (!rc) rc = run_shade(h, P.in(), (const int32_t *)dmeas.p, nc, max_ray_len, ior_env, true);
        if (rc) break;
        ShadeOutPtrs o = shade_ptrs(h, true);
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { rc = set_err(h, LPC_E_HIP, std::string("bounce: ") + hipGetErrorString(e)); break; }
        if ((rc = check_qerr(h)) != 0) break;
        auto d2h = [&](void *dst, const void *src, size_t bytes) {
            if (!rc && dst && hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess)
                rc = set_err(h, LPC_E_HIP, "bounce: D2H");
        };
        auto pack = [&](float *dst4, const float *x, const float *y, const float *z) {
            hipLaunchKernelGGL(k_pack4, dim3(grid1(nc)), dim3(256), 0, h->stream, nc, x, y, z,
                               (float4 *)h->w_stage.p);
            if (hipStreamSynchronize(h->stream) != hipSuccess) { rc = set_err(h, LPC_E_HIP, "pack"); return; }
            d2h(dst4 + 4 * base, h->w_stage.p, (size_t)nc * 16);
        };
        RETIF(dalloc(h, h->w_stage, (size_t)nc * 16));
        pack(dest4, o.destx, o.desty, o.destz);
        pack(r_dir4, o.rdx, o.rdy, o.rdz);
        pack(t_dir4, o.tdx, o.tdy, o.tdz);
        d2h(pow + base, o.pw, (size_t)nc * 4);
        d2h(meas + base, o.meas, (size_t)nc * 4);
        d2h(isect_mid + base, o.imid, (size_t)nc * 4);
        d2h(r_pow + base, o.rpw, (size_t)nc * 4);
        d2h(r_meas + base, o.rms, (size_t)nc * 4);
        d2h(t_pow + base, o.tpw, (size_t)nc * 4);
        d2h(t_meas + base, o.tms, (size_t)nc * 4);
        if (n1_mid) d2h(n1_mid + base, o.n1, (size_t)nc * 4);
        if (n2_mid) d2h(n2_mid + base, o.n2, (size_t)nc * 4);
        if (entering) d2h(entering + base, o.ent, (size_t)nc * 4);
        if (isect_idx) d2h(isect_idx + base, o.iidx, (size_t)nc * 4);
    }
    if (h->prof.on) { (void)hipStreamSynchronize(h->stream); prof_resolve(h); }
    return rc;
}

// ---- reference-kernel drop-ins ------------------------------------------------
int lpc_intersect(lpc_handle *h, int64_t n, const float *dev_origin4, const float *dev_dir4,
                  float max_ray_len, float *dev_tmin, int32_t *dev_cnt, int32_t *dev_itmp)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (n < 0 || !dev_origin4 || !dev_dir4 || !dev_tmin || !dev_cnt || !dev_itmp)
        return set_err(h, LPC_E_ARG, "intersect: missing buffer");
    if (n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t C = std::min(n, chunk_rays(h));
    RETIF(ensure_ws(h, C));
    float *s = (float *)h->w_soa.p;
    const size_t Cw = (size_t)h->ws_rays;
    for (int64_t base = 0; base < n; base += C) {
        const int64_t nc = std::min(C, n - base);
        unpack_rays(h->stream, nc, (const float4 *)dev_origin4 + base, (const float4 *)dev_dir4 + base, s, Cw);
        RaysIn in = soa_rows<RaysIn>((const float *)s, (int64_t)Cw);
        in.pw = nullptr; in.pmid = nullptr;
        IsectOut io;
        const int64_t b = base * h->scene.K;
        RETIF(run_intersect(h, IsectIn{in, nc, max_ray_len, INFINITY, dev_tmin + b, dev_itmp + b, dev_cnt + b}, &io));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    RETIF(check_qerr(h));
    if (h->prof.on) prof_resolve(h);
    return 0;
}

int lpc_intersect_postproc(lpc_handle *h, int64_t n, const float *dev_origin4,
                           const float *dev_dir4, float *dev_dest4, const int32_t *dev_prev_mid,
                           int32_t *dev_n1_mid, int32_t *dev_n2_mid, int32_t *dev_entering,
                           int32_t *dev_isect_mid, int32_t *dev_isect_idx,
                           const float *dev_tmin, const int32_t *dev_cnt,
                           const int32_t *dev_itmp, float max_ray_len)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (n < 0 || !dev_origin4 || !dev_dir4 || !dev_dest4 || !dev_prev_mid || !dev_n1_mid ||
        !dev_n2_mid || !dev_entering || !dev_isect_mid || !dev_isect_idx || !dev_tmin ||
        !dev_cnt || !dev_itmp)
        return set_err(h, LPC_E_ARG, "intersect_postproc: missing buffer");
    if (n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    PostprocAosArgs A;
    A.n = n; A.K = h->scene.K;
    A.origin = (const float4 *)dev_origin4; A.dir = (const float4 *)dev_dir4;
    A.dest = (float4 *)dev_dest4; A.prev_mid = dev_prev_mid;
    A.n1 = dev_n1_mid; A.n2 = dev_n2_mid; A.entering = dev_entering;
    A.imid = dev_isect_mid; A.iidx = dev_isect_idx;
    A.tmin = dev_tmin; A.cnt = dev_cnt; A.itmp = dev_itmp;
    A.mat_type = (const int32_t *)h->scene.d_mat.p; A.max_ray_len = max_ray_len;
    hipLaunchKernelGGL(k_postproc_aos, dim3(grid1(n)), dim3(256), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int lpc_reflect_refract_rays(lpc_handle *h, int64_t n, const float *dev_origin4,
                             const float *dev_dest4, const float *dev_dir4, float *dev_pow,
                             int32_t *dev_meas, const int32_t *dev_n1_mid,
                             const int32_t *dev_n2_mid, float *dev_r_origin4, float *dev_r_dir4,
                             float *dev_r_pow, int32_t *dev_r_meas, float *dev_t_origin4,
                             float *dev_t_dir4, float *dev_t_pow, int32_t *dev_t_meas,
                             const int32_t *dev_isect_mid, const int32_t *dev_isect_idx,
                             float ior_env)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (n < 0 || !dev_origin4 || !dev_dest4 || !dev_dir4 || !dev_pow || !dev_meas ||
        !dev_n1_mid || !dev_n2_mid || !dev_r_origin4 || !dev_r_dir4 || !dev_r_pow ||
        !dev_r_meas || !dev_t_origin4 || !dev_t_dir4 || !dev_t_pow || !dev_t_meas ||
        !dev_isect_mid || !dev_isect_idx)
        return set_err(h, LPC_E_ARG, "reflect_refract_rays: missing buffer");
    if (n == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    FresnelAosArgs A;
    A.n = n;
    A.origin = (const float4 *)dev_origin4; A.dest = (const float4 *)dev_dest4;
    A.dir = (const float4 *)dev_dir4; A.pow = dev_pow; A.meas = dev_meas;
    A.n1 = dev_n1_mid; A.n2 = dev_n2_mid; A.imid = dev_isect_mid; A.iidx = dev_isect_idx;
    A.r_origin = (float4 *)dev_r_origin4; A.r_dir = (float4 *)dev_r_dir4;
    A.t_origin = (float4 *)dev_t_origin4; A.t_dir = (float4 *)dev_t_dir4;
    A.r_pow = dev_r_pow; A.t_pow = dev_t_pow; A.r_meas = dev_r_meas; A.t_meas = dev_t_meas;
    A.mat_type = (const int32_t *)h->scene.d_mat.p; A.ior = (const float *)h->scene.d_ior.p;
    A.refl = (const float *)h->scene.d_refl.p; A.diss = (const float *)h->scene.d_diss.p;
    A.verts = (const float *)h->scene.d_verts.p; A.ior_env = ior_env;
    hipLaunchKernelGGL(k_fresnel_aos, dim3(grid1(n)), dim3(256), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// ---- device-resident trace ------------------------------------------------------
int lpc_set_walk_grid(lpc_handle *h, int64_t blocks)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (blocks != 0 && (blocks < 64 || blocks > (1 << 22))) return set_err(h, LPC_E_ARG, "walk grid out of range");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    h->knobs.walk_grid = blocks ? blocks : kWalkWaves;
    return 0;
}

int lpc_set_chunk(lpc_handle *h, int64_t rays_per_chunk)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (rays_per_chunk < 0) return set_err(h, LPC_E_ARG, "negative chunk");
    h->knobs.chunk = rays_per_chunk;
    return 0;
}

// May the emitted rays' coherence sort be the counting sort (k_bkey..k_bsort2)?
// Its second level runs one block per hi bucket, so it pays only when no bucket
// is large: the hi-digit counts of k_raykey's key that k_ray_scan counted for
// the key window in use.  A collimated beam's few origin cells, or a narrow
// cone's few direction cells, go to rocPRIM (the sort is exact either way).
static bool bsort_fits(int key_lo, int key_hi, int64_t n, const RayScan &S)
{
    const int nbits = key_hi - key_lo;
    if (nbits < 1 || nbits > 16 || n < LPC_MISC_WORDS) return false;
    const int hb = std::min(nbits, LPC_BS_HB), lb = nbits - hb;
    if (lb == 0) return true;                              // one level: no per-bucket pass
    const int w = key_lo + lb == 8 ? 0 : key_lo + lb == 23 ? 1 : -1;
    if (w < 0 || hb != 8) return false;                   // windows k_ray_scan did not count
    uint32_t mx = 0;
    for (int b = 0; b < 256; ++b) mx = std::max(mx, S.hist[w][b]);
    return mx <= (uint32_t)LPC_BS_MAXB;
}

// The analysis of n new rays against the scene's key box (k_ray_scan) on the
// stream, read back into S (one 2 KB copy; no rays: zeros).
static int ray_scan(lpc_handle *h, const RaysIn &in, int64_t n, DBuf &d, RayScan *S)
{
    const Scene &sc = h->scene;
    memset(S, 0, sizeof(RayScan));
    if (n <= 0) return 0;
    RETIF(dalloc(h, d, sizeof(RayScan)));
    HIPCHK(h, hipMemsetAsync(d.p, 0, sizeof(RayScan), h->stream));
    hipLaunchKernelGGL(k_ray_scan, dim3((unsigned)std::min<int64_t>(grid1(n), 2048)), dim3(256), 0, h->stream, in, n,
                       sc.box_lo[0], sc.box_lo[1], sc.box_lo[2], sc.box_scale[0], sc.box_scale[1], sc.box_scale[2],
                       (RayScan *)d.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(S, d.p, sizeof(RayScan), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

// The emitted rays' analysis (k_ray_scan) into the trace state, as the rays in
// I: lpc_trace_set_rays and a staged batch that becomes current.
static int emitted_rays(lpc_handle *h, int64_t n, const RayScan &S, float max_ray_len, float ior_env)
{
    Emitted E;
    E.n_init = n; E.max_ray_len = max_ray_len; E.ior_env = ior_env;
    memcpy(&E.init_dmax2, &S.dmax2_bits, sizeof(double));
    E.pow_nonneg = S.neg_pow == 0u;
    // coherence key bits that can vary over these rays (k_raykey: [origin cell 15 |
    // direction 16]): a point source has one origin cell, a collimated beam one
    // direction, and the sort skips the rest
    const bool same_o = S.diff_o == 0u, same_d = S.diff_d == 0u;
    E.init_key_lo = 0; E.init_key_hi = 31;
    if (same_o) E.init_key_hi = 16;
    if (same_d) E.init_key_lo = 16;
    if (same_o && same_d) { E.init_key_lo = 0; E.init_key_hi = 8; }   // one digit pass
    E.init_bsort = bsort_fits(E.init_key_lo, E.init_key_hi, n, S);
    RETIF(check_dcap(h, E.init_dmax2));             // failed: the previous record went with the scene
    E.ready = true;
    h->emitted = E;
    return lpc_trace_reset(h);
}

int lpc_trace_set_rays(lpc_handle *h, int64_t n, const float *origin4, const float *dir4,
                       const float *pow, float max_ray_len, float ior_env)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (n < 0 || (n > 0 && (!origin4 || !dir4 || !pow))) return set_err(h, LPC_E_ARG, "set_rays: missing buffer");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    RETIF(pop_reserve(h, h->I, std::max<int64_t>(n, 1)));
    if (n > 0) RETIF(upload_rays(h, h->I, n, origin4, dir4, pow, nullptr, false));
    RayScan S;
    RETIF(ray_scan(h, h->I.in(), n, h->d_scan, &S));
    return emitted_rays(h, n, S, max_ray_len, ior_env);
}

int lpc_trace_reset(lpc_handle *h)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(need_rays(h, "trace_reset"));
    HIPCHK(h, hipSetDevice(h->device));
    // the first iteration reads the emitted rays where set_rays put them (I is
    // never written by an iteration: no copy)
    const Emitted &E = h->emitted;
    h->pop = PopState{E.n_init, E.init_dmax2, /*init*/ true, /*traced*/ false, /*emitted*/ true, /*pbox_ok*/ false};
    h->mp_valid = true;                             // until an iteration does not sum it
    h->m_total = 0;                             // measured record emptied (the first iteration resets the counters)
    h->m_inflight = 0;
    // the ledgers go with the measured record (stream-ordered: behind whatever
    // an earlier trace still runs)
    return ledgers_clear(h);
}

// ---- streamed batches of new rays ------------------------------------------
// A staged batch is copied by a helper thread: the caller's (n,4) rows as they
// are (pageable DMA, 36 B per ray cross PCIe; staging them in pinned memory, as
// rows or transposed, measured slower and was removed: DESIGN.md section 7f),
// their unpack, the emitted rays' fills and k_ray_scan, all on the copy stream,
// which first waits for the main-stream work queued when the batch was staged
// (the slot's buffers may hold an earlier batch's emitted rays).  The main
// thread meanwhile traces the batch before it.
static void stage_worker(lpc_handle *h, lpc_handle::RaySlot *s, const float *origin4, const float *dir4,
                         const float *pow, std::array<float, 6> box, bool scan)   // box: the key box lo | scale
{
    auto fail = [&](hipError_t e, const char *what) {
        s->rc = LPC_E_HIP;
        s->err = std::string("stage_rays: ") + what + ": " + hipGetErrorString(e);
    };
    const double t0 = h->knobs.host_prof ? host_us() : 0.0;
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) { fail(e, "hipSetDevice"); return; }
    const int64_t n = s->n;
    hipStream_t cs = h->stage.cstream;
    // the (n,4) rows as they are, from the caller's memory (the runtime's own
    // staging of a pageable copy), unpacked on the device
    float4 *so = (float4 *)s->aos.p, *sd = so + n;
    if ((e = hipMemcpyAsync(so, origin4, (size_t)n * 16, hipMemcpyHostToDevice, cs)) != hipSuccess ||
        (e = hipMemcpyAsync(sd, dir4, (size_t)n * 16, hipMemcpyHostToDevice, cs)) != hipSuccess ||
        (e = hipMemcpyAsync(s->P.f(6), pow, (size_t)n * 4, hipMemcpyHostToDevice, cs)) != hipSuccess) {
        fail(e, "copy");
        return;
    }
    unpack_rays(cs, n, so, sd, s->P.f(0), (size_t)s->P.cap);
    if ((e = hipMemsetD32Async((hipDeviceptr_t)s->P.pmid(), -2, (size_t)n, cs)) != hipSuccess) { fail(e, "fill"); return; }
    if (scan) {                                     // the scene's key box is known: the analysis rides along
        if ((e = hipMemsetAsync(s->scan.p, 0, sizeof(RayScan), cs)) != hipSuccess) { fail(e, "fill"); return; }
        hipLaunchKernelGGL(k_ray_scan, dim3((unsigned)std::min<int64_t>(grid1(n), 2048)), dim3(256), 0, cs, s->P.in(),
                           n, box[0], box[1], box[2], box[3], box[4], box[5], (RayScan *)s->scan.p);
        if ((e = hipGetLastError()) != hipSuccess) { fail(e, "launch"); return; }
        if ((e = hipMemcpyAsync(s->scan_host, s->scan.p, sizeof(RayScan), hipMemcpyDeviceToHost, cs)) != hipSuccess) {
            fail(e, "copy");
            return;
        }
    }
    if ((e = hipEventRecord(s->ev, cs)) != hipSuccess) fail(e, "event");
    if (h->knobs.host_prof) {
        const double t1 = host_us();
        (void)hipEventSynchronize(s->ev);
        fprintf(stderr, "[lpc host] stage: %lld rays, enqueued %.1f us, done %.1f us\n", (long long)n, t1 - t0,
                host_us() - t0);
    }
}

int lpc_trace_stage_rays(lpc_handle *h, int64_t n, const float *origin4, const float *dir4, const float *pow,
                         float max_ray_len, float ior_env)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (n <= 0 || !origin4 || !dir4 || !pow) return set_err(h, LPC_E_ARG, "stage_rays: need n > 0 rays and all buffers");
    if (h->stage.rs_count >= 2) return set_err(h, LPC_E_STATE, "stage_rays: two batches are staged already");
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->stage.cstream) {
        HIPCHK(h, h->stage.cstream.create());
        HIPCHK(h, h->stage.ev_stage.create());
    }
    lpc_handle::RaySlot &s = h->stage.rslot[(h->stage.rs_head + h->stage.rs_count) % 2];
    if (s.th.joinable()) s.th.join();
    if (!s.ev) HIPCHK(h, s.ev.create());
    if (!s.scan_host) HIPCHK(h, s.scan_host.alloc(sizeof(RayScan)));
    // buffers (allocations synchronise; they grow only with the batch size)
    RETIF(pop_reserve(h, s.P, n));
    RETIF(dalloc(h, s.scan, sizeof(RayScan)));
    RETIF(dalloc(h, s.aos, (size_t)n * 32));
    s.n = n;
    s.max_ray_len = max_ray_len;
    s.ior_env = ior_env;
    s.rc = 0;
    s.err.clear();
    s.scan_gen = h->scene.ready ? h->scene_gen : -1;      // no scene yet: the scan runs when the batch is traced
    // the slot's device buffers may hold an earlier batch's emitted rays: the copy
    // stream starts after the main-stream work queued so far
    HIPCHK(h, hipEventRecord(h->stage.ev_stage, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->stage.cstream, h->stage.ev_stage, 0));
    const float *lo = h->scene.box_lo, *sc = h->scene.box_scale;    // by value: the helper outlives this call
    s.th = std::thread(stage_worker, h, &s, origin4, dir4, pow,
                       std::array<float, 6>{lo[0], lo[1], lo[2], sc[0], sc[1], sc[2]}, s.scan_gen >= 0);
    ++h->stage.rs_count;
    return 0;
}

static int trace_run(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                     int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap,
                     bool wait);

int lpc_trace_run_staged_async(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                               int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (!h->stage.rs_count) return set_err(h, LPC_E_STATE, "run_staged: no batch staged (lpc_trace_stage_rays)");
    RETIF(need_scene(h));
    if (mesh_power && mesh_power_cap < h->scene.K)
        return set_err(h, LPC_E_ARG, "trace: mesh_power capacity below the scene's mesh count");
    if (!n_iter || (max_iter > 0 && !per_iter)) return set_err(h, LPC_E_ARG, "trace_run: null output");
    HIPCHK(h, hipSetDevice(h->device));
    lpc_handle::RaySlot &s = h->stage.rslot[h->stage.rs_head];
    if (s.th.joinable()) s.th.join();
    h->stage.rs_head ^= 1;
    --h->stage.rs_count;
    if (s.rc) return set_err(h, s.rc, s.err);
    // the analysis is read on the host (the copy ran during the previous trace);
    // the trace's first kernels wait for the batch on the device
    HIPCHK(h, hipEventSynchronize(s.ev));
    HIPCHK(h, hipStreamWaitEvent(h->stream, s.ev, 0));
    if (s.scan_gen != h->scene_gen)             // staged before this scene: its analysis now, on the stream
        RETIF(ray_scan(h, s.P.in(), s.n, s.scan, s.scan_host));
    std::swap(h->I, s.P);
    RETIF(emitted_rays(h, s.n, *s.scan_host, s.max_ray_len, s.ior_env));
    return trace_run(h, max_iter, power_threshold, per_iter, n_iter, measured_count, mesh_power, mesh_power_cap,
                     false);
}

// All-reduce (sum) of the iteration's stats over the ranks of a sharded trace.
// Slot 0 of every exchange is a failure flag (0 from a healthy rank, 1 from a
// rank that failed locally: xchg_poison), so the data values are free to hold
// NaN -- a trace whose ray powers are NaN keeps iterating exactly as a single
// device (and the reference: NaN < thr is false) does.
#define LPC_XCHG_STATS 6
static int xchg_stats(lpc_handle *h, const lpc_iter_stats &S, lpc_iter_stats *G)
{
    double v[LPC_XCHG_STATS] = {0.0, (double)S.n_in, (double)S.n_reflect, (double)S.n_refract,
                                (double)S.n_measured, S.power_next};
    const double t0 = host_us();
    const int rc = h->xchg(h->xchg_ctx, v, LPC_XCHG_STATS);
    h->xchg_us += host_us() - t0;
    h->xchg_calls += 1;
    if (rc != 0) return set_err(h, LPC_E_STATE, "trace: all-reduce hook failed");
    if (v[0] != 0.0) return set_err(h, LPC_E_STATE, "trace: a peer rank failed (failure flag in the all-reduced stats)");
    G->n_in = (int64_t)v[1]; G->n_reflect = (int64_t)v[2]; G->n_refract = (int64_t)v[3];
    G->n_measured = (int64_t)v[4]; G->power_next = v[5];
    return 0;
}

// A rank that fails locally still takes part in the exchange its peers wait in,
// with the failure flag (slot 0) set: they see it in the sums and fail at once
// (xchg_stats, the trace-end sums) instead of waiting for a rank that left, and
// every rank has made the same number of exchanges.  The flag sits in slot 0 of
// every exchange shape, so the peers see it whichever exchange they are in.  The
// local error stays the one reported.
static void xchg_poison(lpc_handle *h, int32_t n)
{
    if (!h->xchg) return;
    std::vector<double> v((size_t)n, std::numeric_limits<double>::quiet_NaN());
    v[0] = 1.0;
    const std::string keep = h->err;
    (void)h->xchg(h->xchg_ctx, v.data(), n);
    h->err = keep;
}

int lpc_trace_run(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                  int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap)
{
    return trace_run(h, max_iter, power_threshold, per_iter, n_iter, measured_count, mesh_power, mesh_power_cap,
                     true);
}

int lpc_trace_run_async(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                        int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap)
{
    return trace_run(h, max_iter, power_threshold, per_iter, n_iter, measured_count, mesh_power, mesh_power_cap,
                     false);
}

int lpc_trace_rerun_async(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                          int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap)
{
    if (h && mesh_power && mesh_power_cap < h->scene.K)       // before the reset: nothing changed on error
        return set_err(h, LPC_E_ARG, "trace: mesh_power capacity below the scene's mesh count");
    RETIF(lpc_trace_reset(h));
    return trace_run(h, max_iter, power_threshold, per_iter, n_iter, measured_count, mesh_power, mesh_power_cap,
                     false);
}

int lpc_set_allreduce(lpc_handle *h, lpc_allreduce_fn fn, void *ctx)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    h->xchg = fn;
    h->xchg_ctx = ctx;
    return 0;
}

int lpc_trace_global_stats(lpc_handle *h, lpc_iter_stats *per_iter, int32_t cap, int32_t *n_iter)
{
    if (!h || !n_iter) return set_err(h, LPC_E_ARG, "null argument");
    *n_iter = (int32_t)h->gstats.size();
    if (per_iter)
        for (int32_t i = 0; i < std::min(cap, *n_iter); ++i) per_iter[i] = h->gstats[(size_t)i];
    return 0;
}

int lpc_trace_set_min_power(lpc_handle *h, float min_power)
{
    if (!(min_power >= 0.0f) || !std::isfinite(min_power))
        return set_err(h, LPC_E_ARG, "set_min_power: the cutoff must be finite and >= 0");
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (min_power != h->led.min_power) {
        // a prediction made under another cutoff is not reused
        h->hist_r.clear();
        h->hist_iter = -1;
    }
    h->led.min_power = min_power;           // from the next launched iteration
    return 0;
}

int lpc_trace_culled(lpc_handle *h, int64_t *count, double *power, int32_t cap, int32_t *n_iter)
{
    if (!h || !n_iter) return set_err(h, LPC_E_ARG, "null argument");
    if (cap < 0 || (cap > 0 && (!count || !power))) return set_err(h, LPC_E_ARG, "trace_culled: missing buffer");
    RETIF(settle(h));
    const int64_t n = std::min<int64_t>(h->led.it_done, kCullSlots);
    *n_iter = (int32_t)n;
    const int64_t m = std::min<int64_t>(n, cap);
    for (int64_t i = 0; i < m; ++i) { count[i] = 0; power[i] = 0.0; }
    if (m > 0 && h->led.cull.buf.p) {
        HIPCHK(h, hipSetDevice(h->device));
        std::vector<CullSlot> v((size_t)m);
        HIPCHK(h, hipMemcpyAsync(v.data(), h->led.cull.buf.p, (size_t)m * sizeof(CullSlot), hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int64_t i = 0; i < m; ++i) { count[i] = (int64_t)v[(size_t)i].count; power[i] = v[(size_t)i].power; }
    }
    return 0;
}

int lpc_trace_set_budget(lpc_handle *h, int on)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    h->led.budget = on != 0;                // from the next launched iteration
    return 0;
}

static_assert(sizeof(lpc_budget_iter) == sizeof(BudgetRow), "lpc_budget_iter is BudgetRow's layout");

int lpc_trace_budget(lpc_handle *h, lpc_budget_iter *per_iter, int32_t iter_cap, int32_t *n_iter,
                     double *mesh_power, int64_t *mesh_count, int32_t mesh_cap)
{
    if (!h || !n_iter) return set_err(h, LPC_E_ARG, "null argument");
    if (iter_cap < 0 || (iter_cap > 0 && !per_iter)) return set_err(h, LPC_E_ARG, "trace_budget: missing buffer");
    if ((mesh_power || mesh_count) && mesh_cap < h->scene.K)
        return set_err(h, LPC_E_ARG, "trace_budget: mesh capacity below the scene's mesh count");
    RETIF(settle(h));
    const Ledgers &G = h->led;
    const int64_t n = G.bud_seen ? std::min<int64_t>(G.it_done, kCullSlots) : 0;
    *n_iter = (int32_t)n;
    const int64_t m = std::min<int64_t>(n, iter_cap);
    if (m > 0) memset(per_iter, 0, (size_t)m * sizeof(lpc_budget_iter));
    if (m > 0 && G.bud.dirty) {         // (waited for with the tables: rows and tables are dirty together)
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpyAsync(per_iter, G.bud.buf.p, (size_t)m * sizeof(BudgetRow), hipMemcpyDeviceToHost, h->stream));
    }
    return staged_read(h, G.bud_mesh, (int64_t)h->scene.K * 4, {mesh_power, mesh_count});
}

int lpc_trace_set_surface(lpc_handle *h, int on)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    h->led.surface = on != 0;               // from the next launched iteration
    return 0;
}

static_assert(LPC_SURF_LDS == LPC_SURFACE_LDS_ENTRIES, "lpc.h states k_surface_sum's LDS table size");
static_assert((LPC_SURF_LDS & (LPC_SURF_LDS - 1)) == 0, "k_surface_sum maps a triangle by its low bits");

int lpc_trace_surface(lpc_handle *h, double *incident, double *deposited, int64_t *count, int64_t tri_cap,
                      int64_t *tri_count)
{
    if (!h || !tri_count) return set_err(h, LPC_E_ARG, "null argument");
    RETIF(need_scene(h));
    const int64_t M = h->scene.M;
    *tri_count = M;                     // (also where the arrays are refused: the caller learns the size)
    if ((incident || deposited || count) && tri_cap < M)
        return set_err(h, LPC_E_ARG, "trace_surface: triangle capacity below the scene's triangle count");
    RETIF(settle(h));
    return staged_read(h, h->led.surf, M, {incident, deposited, count});
}

static_assert(LPC_VOL_LDS == LPC_VOLUME_LDS_ENTRIES, "lpc.h states k_volume_sum's LDS table size");
static_assert((LPC_VOL_LDS & (LPC_VOL_LDS - 1)) == 0, "k_volume_sum maps a voxel by its low bits");

// A grid as lpc.h admits it -> its voxel count, or 0.
static int64_t volume_grid(const double *lo3, const double *hi3, const int32_t *dims3, lpc::VolumeGrid *G)
{
    int64_t V = 1;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo3[k]) || !std::isfinite(hi3[k]) || !(lo3[k] < hi3[k]) || !std::isfinite(hi3[k] - lo3[k]))
            return 0;
        if (dims3[k] < 1 || dims3[k] > 1024) return 0;
        G->lo[k] = lo3[k]; G->hi[k] = hi3[k]; G->n[k] = dims3[k];
        V *= dims3[k];
    }
    G->pad = 0;
    return V <= ((int64_t)1 << 27) ? V : 0;
}

int lpc_trace_set_volume(lpc_handle *h, const double *lo3, const double *hi3, const int32_t *dims3)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    Ledgers &G = h->led;
    if (!lo3) { G.volume = false; return 0; }       // from the next launched iteration; the grid stays readable
    if (!hi3 || !dims3) return set_err(h, LPC_E_ARG, "trace_set_volume: null argument");
    lpc::VolumeGrid g = {};
    const int64_t V = volume_grid(lo3, hi3, dims3, &g);
    if (!V)
        return set_err(h, LPC_E_ARG, "trace_set_volume: a grid needs finite lo < hi, dims in 1..1024 and at most 2^27 voxels");
    if (memcmp(&g, &G.vgrid, sizeof(g)) != 0 && G.vol.dirty) {      // what was booked belongs to another grid
        HIPCHK(h, hipSetDevice(h->device));
        if (G.vol.buf.p) HIPCHK(h, hipMemsetAsync(G.vol.buf.p, 0, G.vol.buf.bytes, h->stream));
        G.vol.dirty = false;
    }
    G.vgrid = g; G.vV = V;
    G.volume = true;
    return 0;
}

int lpc_trace_volume(lpc_handle *h, double *deposited, int64_t cap, int32_t *dims3, double *outside, int64_t *segments)
{
    if (!h || !dims3) return set_err(h, LPC_E_ARG, "null argument");
    const Ledgers &G = h->led;
    for (int k = 0; k < 3; ++k) dims3[k] = G.vgrid.n[k];
    const int64_t V = G.vV;
    if (deposited && cap < V) return set_err(h, LPC_E_ARG, "trace_volume: capacity below the grid's voxel count");
    RETIF(settle(h));
    if (deposited && V > 0) memset(deposited, 0, (size_t)V * 8);
    double tail[2] = {0.0, 0.0};
    const StagedTable &T = G.vol;
    if (T.dirty && T.live() && T.n == V + 2) {
        HIPCHK(h, hipSetDevice(h->device));
        if (deposited)
            HIPCHK(h, hipMemcpyAsync(deposited, T.total(), (size_t)V * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(tail, T.total() + V, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (outside) *outside = tail[0];
    if (segments) *segments = (int64_t)llrint(tail[1]);
    return 0;
}

int lpc_volume_segment_host(const double *lo3, const double *hi3, const int32_t *dims3, const double *O3,
                            const double *E3, double a, double D, int64_t *idx, double *share, int64_t cap, int64_t *n)
{
    if (!lo3 || !hi3 || !dims3 || !O3 || !E3 || !n || cap < 0 || (cap > 0 && (!idx || !share)))
        return set_err(nullptr, LPC_E_ARG, "volume_segment_host: bad argument");
    lpc::VolumeGrid g = {};
    if (!volume_grid(lo3, hi3, dims3, &g)) return set_err(nullptr, LPC_E_ARG, "volume_segment_host: bad grid");
    int64_t m = 0;
    auto book = [&](int32_t v, double s) {
        if (m < cap) { idx[m] = v; share[m] = s; }
        ++m;
    };
    lpc::VolumeWalk w;
    lpc::volume_begin(w, g, O3, E3, a, D, book);
    while (!lpc::volume_step(w, g, book)) {}
    *n = m;                             // (beyond cap: the count needed, the first cap intervals written)
    return 0;
}

int lpc_shm_comm_open(const char *name, int32_t rank, int32_t world, int32_t create, lpc_shm_comm **out)
{
    if (!out) return set_err(nullptr, LPC_E_ARG, "shm comm: null output");
    std::string err;
    lpcc::ShmComm *c = nullptr;
    if (lpcc::shm_open_comm(name, rank, world, create, &c, &err) != 0) return set_err(nullptr, LPC_E_ARG, err);
    *out = (lpc_shm_comm *)c;
    return 0;
}

int lpc_shm_comm_unlink(lpc_shm_comm *c)
{
    if (!c) return set_err(nullptr, LPC_E_ARG, "shm comm: null");
    lpcc::shm_unlink_comm((lpcc::ShmComm *)c);
    return 0;
}

int lpc_shm_allreduce(void *comm, double *vals, int32_t n)
{
    lpcc::ShmComm *c = (lpcc::ShmComm *)comm;
    if (!c) return set_err(nullptr, LPC_E_ARG, "shm comm: null");
    if (lpcc::shm_allreduce(c, vals, n) != 0)
        return set_err(nullptr, LPC_E_STATE, c->err.empty() ? "shm comm: bad argument" : c->err);
    return 0;
}

int lpc_shm_comm_abort(lpc_shm_comm *c)
{
    if (!c) return set_err(nullptr, LPC_E_ARG, "shm comm: null");
    lpcc::shm_abort((lpcc::ShmComm *)c, "shm comm: aborted by this rank");
    return 0;
}

int lpc_shm_comm_close(lpc_shm_comm *c)
{
    lpcc::shm_close_comm((lpcc::ShmComm *)c);
    return 0;
}

int lpc_sync(lpc_handle *h)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    return settle(h);
}

int lpc_trace_population(lpc_handle *h, int64_t *n)
{
    if (!h || !n) return set_err(h, LPC_E_ARG, "null argument");
    *n = h->pop.n;
    return 0;
}

static int ensure_measured(lpc_handle *h, int64_t need)
{
    if (need <= h->m_cap) return 0;
    // the first reservation takes twice the need: a trace's next iterations then
    // append without the growth copy (which waits for the stream)
    int64_t cap = std::max<int64_t>(h->m_cap ? need : 2 * need, std::max<int64_t>(2 * h->m_cap, 1 << 16));
    DBuf nb;
    RETIF(dalloc(h, nb, (size_t)cap * 5 * 4));
    if (h->m_cap > 0) {         // all old rows: an iteration still in flight may append past m_total
        for (int k = 0; k < 5; ++k)
            HIPCHK(h, hipMemcpyAsync((char *)nb.p + (size_t)k * cap * 4,
                                     (char *)h->m_buf.p + (size_t)k * h->m_cap * 4,
                                     (size_t)h->m_cap * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    h->m_buf = std::move(nb);
    h->m_cap = cap;
    return 0;
}

// Wait (spinning) until k_scan / k_stage_move has published the counters of the
// iteration with sequence number `seq` in its mapped ring slot; the stream keeps
// running.  A stream that fails or finishes without publishing is reported.
static int wait_mapped_acc(lpc_handle *h, unsigned seq, DevAcc *out)
{
    DevAcc *slot = h->acc_map + seq % kAccRing;
    volatile DevAcc *m = slot;
    for (uint64_t i = 1;; ++i) {
        if (__atomic_load_n(&slot->seq, __ATOMIC_ACQUIRE) == seq) break;
        if ((i & 255u) == 0u) {
            const hipError_t e = hipStreamQuery(h->stream);
            if (e == hipSuccess) {
                if (__atomic_load_n(&slot->seq, __ATOMIC_ACQUIRE) == seq) break;
                return set_err(h, LPC_E_HIP, "iteration counters were not published");
            }
            if (e != hipErrorNotReady) return set_err(h, LPC_E_HIP, std::string("trace: ") + hipGetErrorString(e));
        }
        __builtin_ia32_pause();
    }
    out->nR = m->nR; out->nT = m->nT; out->m_total = m->m_total; out->nM_iter = m->nM_iter;
    out->pow_next = m->pow_next; out->dmax2_bits = m->dmax2_bits; out->qerr = m->qerr;
    out->seq = m->seq; out->pneg = m->pneg;
    for (int k = 0; k < LPC_MP_MAX; ++k) out->mpow[k] = m->mpow[k];
    return 0;
}

// An enqueued iteration whose counters have not been read yet.
struct Pending {
    int64_t n_in = 0;           // its population (-1: device-sized, known once the iteration before is read)
    unsigned seq = 0;           // mapped ring slot / sequence number (early)
    bool early = false;         // counters through the mapped ring (else copy + sync)
    bool fused = false;         // traced (its children come out in traced order), k_shade_stage +
                                //   k_stage_move: it wrote the next IterCtl entry
    bool mp_fused = false;      // it summed the measured power per measure mesh
    bool ds = false;            // device-sized (speculative)
    bool empty = false;         // nothing to do (n_in 0, host-sized)
    int64_t n_bound = 0;        // device-sized: population bound
    double thr = -INFINITY;     // fused: the stop threshold its k_stage_move applied (IterPlan::thr)
    int64_t slot = 0;           // its slot in the trace's ledgers: the iterations collected at its enqueue, one
                                //   more for a device-sized one (the iteration before it is still uncollected)
    LedgerSet on;               // the ledgers it ran with: their staging tables of the slot's parity join the
                                //   trace's when it is collected
    PopState before;            // the population's role before its enqueue (undo of a discarded speculative iteration)
};

// A results export (lpc_trace_iterate_export): the caller's host block and
// whether it holds the origins.  Host layout over the iteration's N rays:
// [origin (N,4) if org][dest (N,4)][pow (N)][meas (N)].
struct ExportSpec {
    char *host = nullptr;
    int org = 0;
};

// One chunk's export: k_export packs it into a staging buffer in the host
// layout, the export stream copies it to the caller's block (one DMA when the
// chunk is the whole population) while the main stream runs on.  Two staging
// buffers alternate; the main stream waits for a buffer's last copy before
// packing into it again.
static int export_chunk(lpc_handle *h, const RaysIn &in, const ShadeOutPtrs &o, int64_t nc, int64_t base,
                        int64_t N, const ExportSpec &X)
{
    if (!h->xp.xstream) {
        HIPCHK(h, h->xp.xstream.create());
        for (int k = 0; k < 2; ++k) {
            HIPCHK(h, h->xp.ev_xready[k].create());
            HIPCHK(h, h->xp.ev_xdone[k].create());
        }
    }
    const int par = h->xp.xpar;
    h->xp.xpar ^= 1;
    const size_t orow = X.org ? 16 : 0;
    const size_t row = orow + 16 + 4 + 4;
    if (h->xp.xst[par].bytes < (size_t)nc * row && h->xp.xdone_rec[par])
        HIPCHK(h, hipEventSynchronize(h->xp.ev_xdone[par]));   // its last copy ends before it is freed
    RETIF(dalloc(h, h->xp.xst[par], (size_t)nc * row));
    if (h->xp.xdone_rec[par]) HIPCHK(h, hipStreamWaitEvent(h->stream, h->xp.ev_xdone[par], 0));
    char *d = (char *)h->xp.xst[par].p;
    float4 *xo = (float4 *)d;
    float4 *xd = (float4 *)(d + (size_t)nc * orow);
    float *xp = (float *)(d + (size_t)nc * (orow + 16));
    int32_t *xm = (int32_t *)(d + (size_t)nc * (orow + 20));
    hipLaunchKernelGGL(k_export, dim3(grid1(nc)), dim3(256), 0, h->stream, nc, in, o, X.org, xo, xd, xp, xm);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->xp.ev_xready[par], h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->xp.xstream, h->xp.ev_xready[par], 0));
    const double hm = h->knobs.host_prof ? host_us() : 0.0;
    // the copy into the caller's pinned block: a copy kernel writing the mapped
    // block over PCIe (round 5: hipMemcpyAsync into a block stalled the host 4-15 ms
    // on the block's first asynchronous copy, whatever primed it, DESIGN.md
    // section 7e), or a DMA copy when the block is not device-mapped / aligned
    auto copy_out = [&](char *host, const char *dev, size_t bytes) -> int {
        void *hdev = nullptr;
        if (hipHostGetDevicePointer(&hdev, host, 0) == hipSuccess && hdev && (((uintptr_t)hdev | (uintptr_t)dev) & 15u) == 0) {
            hipLaunchKernelGGL(k_copy_host, dim3(1024), dim3(256), 0, h->xp.xstream, (const lpc_u4 *)dev, (lpc_u4 *)hdev,
                               (int64_t)(bytes / 16), (int64_t)bytes);
            HIPCHK(h, hipGetLastError());
        } else {
            HIPCHK(h, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->xp.xstream));
        }
        return 0;
    };
    if (nc == N) {
        RETIF(copy_out(X.host, d, (size_t)nc * row));
        if (h->knobs.host_prof)
            fprintf(stderr, "[lpc host]   export copy %.1f us (host %p, %zu B)\n", host_us() - hm, (void *)X.host,
                    (size_t)nc * row);
    } else {                                                    // chunk: each section at its rays' offset
        size_t hoff = 0, doff = 0;
        const size_t elt[4] = {orow, 16, 4, 4};
        for (int k = 0; k < 4; ++k) {
            if (elt[k] == 0) continue;
            RETIF(copy_out(X.host + hoff + (size_t)base * elt[k], d + doff, (size_t)nc * elt[k]));
            hoff += (size_t)N * elt[k];
            doff += (size_t)nc * elt[k];
        }
    }
    HIPCHK(h, hipEventRecord(h->xp.ev_xdone[par], h->xp.xstream));
    h->xp.xdone_rec[par] = true;
    h->xp.x_inflight = true;
    return 0;
}

// Where an iteration's per-ray results go (iter_enqueue).  Empty: nowhere, and the
// iteration runs fused, in traced order.
struct IterOut {
    float *origin4 = nullptr, *dest4 = nullptr, *pow = nullptr;
    int32_t *meas = nullptr;
    float *next_pow = nullptr;              // the kept children's power (iter_collect copies it)
    const ExportSpec *X = nullptr;          // results export (lpc_trace_iterate_export)
    bool per_ray() const { return origin4 || dest4 || pow || meas; }
};

// The ledgers of one enqueued iteration: which are on, the fate records the
// shading writes for the budget or the map (tri: their seventh array, surface
// map on, else NULL), and the sum kernels' arguments (off: zeros).
struct LedgerPlan {
    LedgerSet on;
    BudgetRec R = {};
    int32_t *tri = nullptr;
    float *dest = nullptr;                  // arrays eight to ten (volume map on, else NULL)
    CullSumArgs CS = {};
    BudgetSumArgs BS = {};
    SurfaceSumArgs SS = {};
    VolumeSumArgs VS = {};
    uint32_t rec_mask() const { return (tri ? LPC_REC_TRI : 0u) | (dest ? LPC_REC_DEST : 0u); }
};

// What the chunks of one enqueued iteration share.
struct IterPlan {
    int64_t N = 0, C = 0;                   // the population (device-sized: its bound), rays per chunk
    const DevSize *ds = nullptr;
    const long long *nd() const { return ds ? ds->nd : nullptr; }
    // fused: the stop threshold k_stage_move writes into the next IterCtl entry.
    // Only a device-sized iteration reads an entry, and only the one written by
    // the iteration enqueued immediately before it, which is trace_run's own:
    // what the other callers pass (-INFINITY) reaches no launch.
    double thr = -INFINITY;
    DevAcc *host_acc = nullptr;             // early: the mapped ring slot the counters are published to
    unsigned seq = 0;
    bool want_box = false;                  // fused: the chunks write the children's origin box (d_pbox)
    LedgerPlan L;                           // the ledgers it runs with (ledgers_setup)
};

// The fate records of one chunk, for the ledgers that read them: six arrays of
// ws_rays, the hit triangle with the surface map on, dest with the volume map
// on (at fixed positions: the hit triangle's array is then there, written or not).
static int fate_records(lpc_handle *h, LedgerPlan *L)
{
    const size_t C = (size_t)h->ws_rays;
    RETIF(dalloc(h, h->led.w_rec, (L->on.vol ? 10 : L->on.surf ? 7 : 6) * C * 4));
    float *f = (float *)h->led.w_rec.p;
    L->R.dn = (int32_t *)f; L->R.hit = (int32_t *)(f + C);
    L->R.pin = f + 2 * C; L->R.p = f + 3 * C; L->R.kr = f + 4 * C; L->R.kt = f + 5 * C;
    if (L->on.surf) L->tri = (int32_t *)(f + 6 * C);
    if (L->on.vol) L->dest = f + 7 * C;
    return 0;
}

// The ledgers of an iteration about to be enqueued.  It books into slot P->slot:
// a row of the per-iteration ledgers, and by the slot's parity one of the two
// staging tables.  Both are zeroed here, before the iteration's first chunk
// (k_cull_sum instead writes its slot on the first chunk): a re-run iteration
// starts from zero again, and a dropped speculative iteration's sums never reach
// the trace's tables (ledgers_commit adds a kept iteration's).  The surface map
// has no per-iteration rows and runs past kCullSlots iterations.
static int ledgers_setup(lpc_handle *h, IterPlan *I, Pending *P)
{
    Ledgers &G = h->led;
    LedgerPlan &L = I->L = LedgerPlan();
    const LedgerSet on = P->on = L.on = LedgerSet{G.min_power > 0.0f, G.budget, G.surface, G.volume};
    const int64_t slot = P->slot;
    const int par = (int)(slot & 1);
    if ((on.cut || on.bud) && slot >= kCullSlots)
        return set_err(h, LPC_E_STATE, std::string("trace: the ") + (on.cut ? "culled-power ledger" : "power budget") +
                                           " holds " + std::to_string(kCullSlots) + " iterations");
    if (on.cut) {                       // this launch's per-tile culled sums and the slot
        RETIF(ledger_shape(h, G.cull, (size_t)kCullSlots * sizeof(CullSlot)));
        const size_t nt_ws = ((size_t)h->ws_rays + LPC_ST_TILE - 1) / LPC_ST_TILE;
        RETIF(dalloc(h, G.w_cull, nt_ws * (8 + 4) + 64));
        L.CS.cp = (const double *)G.w_cull.p;
        L.CS.cc = (const uint32_t *)(L.CS.cp + nt_ws);
        L.CS.slot = G.cull.row<CullSlot>(slot);
        G.cull.dirty = true;
    }
    if (on.rec()) RETIF(fate_records(h, &L));
    if (on.bud) {                       // the row, and the per-mesh staging table [K][4]: power, count
        RETIF(ledger_shape(h, G.bud, (size_t)kCullSlots * sizeof(BudgetRow)));
        RETIF(staged_shape(h, G.bud_mesh, (int64_t)h->scene.K * 4));
        double *st = G.bud_mesh.staging(par);
        L.BS.R = L.R;
        L.BS.mat_type = (const int32_t *)h->scene.d_mat.p;
        L.BS.K = h->scene.K;
        L.BS.row = G.bud.row<BudgetRow>(slot);
        L.BS.mp = st; L.BS.mc = (unsigned long long *)G.bud_mesh.col(st, 1);
        HIPCHK(h, hipMemsetAsync(L.BS.row, 0, sizeof(BudgetRow), h->stream));
        RETIF(staged_zero(h, G.bud_mesh, par));
        G.bud.dirty = G.bud_mesh.dirty = true;
    }
    if (on.surf) {                      // the per-triangle staging table [M]: incident, deposited, count
        StagedTable &T = G.surf;
        RETIF(staged_shape(h, T, h->scene.M));
        double *st = T.staging(par);
        L.SS.R = L.R; L.SS.tri = L.tri;
        L.SS.mat_type = (const int32_t *)h->scene.d_mat.p;
        L.SS.K = h->scene.K; L.SS.M = h->scene.M;
        L.SS.inc = st; L.SS.dep = T.col(st, 1); L.SS.cnt = (unsigned long long *)T.col(st, 2);
        RETIF(staged_zero(h, T, par));
        T.dirty = true;
    }
    if (on.vol) {                       // the per-voxel staging table [V + 2]: the voxels, outside, segments
        StagedTable &T = G.vol;
        RETIF(staged_shape(h, T, G.vV + 2));
        const size_t C = (size_t)h->ws_rays;
        L.VS.dn = L.R.dn; L.VS.pin = L.R.pin; L.VS.p = L.R.p;
        L.VS.ex = L.dest; L.VS.ey = L.dest + C; L.VS.ez = L.dest + 2 * C;
        L.VS.diss = (const float *)h->scene.d_diss.p;
        L.VS.K = h->scene.K;
        L.VS.G = G.vgrid; L.VS.V = G.vV;
        L.VS.dep = T.staging(par);
        RETIF(staged_zero(h, T, par));
        T.dirty = true;
    }
    return 0;
}

// A chunk's sums into the iteration's ledgers: the culled sums of the
// compaction's tiles (`tile` rays each; off the counters' publication) and the
// sums over the fate records.  A fused chunk takes both at its end; a plain
// chunk has its records after the shading and its tiles after k_count.  in: the
// chunk's rays as the shading read them (the volume map's origins; on this
// stream nothing writes those rows before the next chunk's or iteration's
// intersect stage).
enum : unsigned { kSumCulled = 1, kSumRecords = 2 };
static void ledgers_sum(lpc_handle *h, const IterPlan &I, const RaysIn &in, int64_t base, int64_t nc, int tile,
                        unsigned what)
{
    const LedgerPlan &L = I.L;
    if ((what & kSumCulled) && L.on.cut) {
        CullSumArgs CS = L.CS;
        CS.first = base == 0 ? 1 : 0;
        CS.ntiles = (nc + tile - 1) / tile; CS.tile = tile; CS.nd = I.nd();
        hipLaunchKernelGGL(k_cull_sum, dim3(1), dim3(256), 0, h->stream, CS);
    }
    if (!(what & kSumRecords)) return;
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nc + 255) / 256, 1024));
    if (L.on.bud) {
        BudgetSumArgs BS = L.BS;
        BS.n = nc; BS.nd = I.nd();
        hipLaunchKernelGGL(k_budget_sum, dim3(nb), dim3(256), 0, h->stream, BS);
    }
    if (L.on.surf) {
        SurfaceSumArgs SS = L.SS;
        SS.n = nc; SS.nd = I.nd();
        hipLaunchKernelGGL(k_surface_sum, dim3(nb), dim3(256), 0, h->stream, SS);
    }
    if (L.on.vol) {
        VolumeSumArgs VS = L.VS;
        VS.ox = in.ox; VS.oy = in.oy; VS.oz = in.oz;
        VS.n = nc; VS.nd = I.nd();
        hipLaunchKernelGGL(k_volume_sum, dim3(nb), dim3(256), 0, h->stream, VS);
    }
}

// A collected iteration's staging tables into the trace's (the kernels differ:
// each skips the entries its own count column leaves at zero).
static int ledgers_commit(lpc_handle *h, const Pending &P)
{
    const int par = (int)(P.slot & 1);
    const StagedTable &B = h->led.bud_mesh, &S = h->led.surf, &W = h->led.vol;
    if (P.on.bud && B.live()) {
        double *tot = B.total(), *st = B.staging(par);
        hipLaunchKernelGGL(k_budget_commit, dim3((unsigned)std::min<int64_t>((B.n + 255) / 256, 64)), dim3(256), 0,
                           h->stream, tot, (unsigned long long *)B.col(tot, 1), (const double *)st,
                           (const unsigned long long *)B.col(st, 1), (int)B.n);
        HIPCHK(h, hipGetLastError());
        h->inflight = true;
    }
    if (P.on.surf && S.live()) {
        double *tot = S.total(), *st = S.staging(par);
        hipLaunchKernelGGL(k_surface_commit, dim3((unsigned)std::min<int64_t>((S.n + 255) / 256, 1024)), dim3(256), 0,
                           h->stream, tot, S.col(tot, 1), (unsigned long long *)S.col(tot, 2), (const double *)st,
                           (const double *)S.col(st, 1), (const unsigned long long *)S.col(st, 2), (int)S.n);
        HIPCHK(h, hipGetLastError());
        h->inflight = true;
    }
    if (P.on.vol && W.live()) {
        hipLaunchKernelGGL(k_volume_commit, dim3((unsigned)std::min<int64_t>((W.n + 255) / 256, 4096)), dim3(256), 0,
                           h->stream, W.total(), (const double *)W.staging(par), W.n);
        HIPCHK(h, hipGetLastError());
        h->inflight = true;
    }
    return 0;
}

// One chunk of a traced iteration: shade + staged compaction, two kernels
// (k_shade_stage, k_stage_move; several chunks: each places its rows after the
// earlier chunks', refracted rows staged in T, k_append at the end).  tmask: the
// written-slot masks of the chunk's run_intersect.
static int enqueue_fused_chunk(lpc_handle *h, const IterPlan &I, const RaysIn &in, uint32_t *tmask, int64_t base,
                               int64_t nc)
{
    const DevSize *ds = I.ds;
    const size_t mc = (size_t)h->m_cap;
    float *mf = (float *)h->m_buf.p;
    const size_t Cs = (size_t)h->ws_rays;
    const int64_t ntc = (int64_t)((Cs + LPC_ST_TILE - 1) / LPC_ST_TILE);   // staging tile arrays' stride
    // device-sized: grid from the expected size (grid-stride over the actual tiles)
    const int64_t ng_rays = ds ? std::max<int64_t>(1, std::min(ds->pred, nc)) : nc;
    const int64_t nt = (ng_rays + LPC_ST_TILE - 1) / LPC_ST_TILE;
    const int64_t nt_max = (nc + LPC_ST_TILE - 1) / LPC_ST_TILE;     // tiles the launch may touch
    StageArgs G;
    G.S = shade_args(h, in, nullptr, nc, h->emitted.max_ray_len, h->emitted.ior_env, false);
    G.nd = I.nd();
    G.stR = (float *)h->w_shf.p; G.stT = (float *)h->w_shi.p;   // the 20 shade-output arrays hold the staging rows
    G.stM = (float *)h->w_soa.p; G.cst = (int64_t)Cs;
    G.tpow = (double *)h->w_fc.p; G.tcnt = (uint32_t *)(G.tpow + ntc); G.tdm = G.tcnt + ntc;
    G.skey = (unsigned long long *)h->w_key.p; G.scnt = (int32_t *)h->w_sc.p;
    // measured power per measure mesh summed on the way (no k_mesh_sum at the trace end)
    G.nmp = h->scene.meas_meshes.size() <= (size_t)LPC_MP_MAX ? (int)h->scene.meas_meshes.size() : 0;
    for (int m = 0; m < LPC_MP_MAX; ++m) G.mpm[m] = m < G.nmp ? h->scene.meas_meshes[(size_t)m] : -1;
    G.tmp = (double *)(G.tdm + ntc);            // 16 ntc bytes in: 8-aligned
    const int64_t ng = (nt_max + LPC_ST_GROUP - 1) / LPC_ST_GROUP;
    unsigned long long *gs = (unsigned long long *)h->w_gsum.p;
    const GroupWords::Turn gt = h->groups.turn(ng);     // this launch's k_shade_stage adds into its first ng groups
    G.gsum = gs + gt.cur;
    G.tmask = tmask;
    G.single = tmask && h->knobs.shade_fast ? 1u : 0u;
    G.refr = h->scene.refr;
    G.tbox = I.want_box ? (uint32_t *)h->w_tbox.p : nullptr;
    G.cut = h->led.min_power; G.tcc = (uint32_t *)I.L.CS.cc; G.tcp = (double *)I.L.CS.cp;
    G.bud = I.L.R; G.bud_tri = I.L.rec_mask();          // (the records' stride is cst: both are ws_rays)
    // (this nesting keeps the instantiations in their order in the code object;
    // the power budget's come after the others)
    auto launch_stage = [&](auto bud) {
        with_bool(I.L.on.cut, [&](auto ct) {
            with_bool(ds != nullptr, [&](auto dsz) {
                with_ku(h->scene.K, [&](auto ku) {
                    hipLaunchKernelGGL((k_shade_stage<decltype(ku)::value, decltype(dsz)::value, decltype(ct)::value,
                                                      decltype(bud)::value>),
                                       dim3((unsigned)nt), dim3(LPC_ST_TILE), 0, h->stream, G);
                });
            });
        });
    };
    if (!I.L.on.rec()) launch_stage(std::false_type{});
    else launch_stage(std::true_type{});
    MoveArgs M;
    M.ntiles = nt_max; M.ngroups = ng;
    M.stR = G.stR; M.stT = G.stT; M.stM = G.stM; M.cst = G.cst;
    M.tcnt = G.tcnt; M.tpow = G.tpow; M.tdm = G.tdm; M.nmp = G.nmp; M.tmp = G.tmp; M.gsum = G.gsum;
    M.popR = h->B.f(0); M.capR = h->B.cap;
    M.mrec = mf; M.capM = (int64_t)mc; M.m_base = (unsigned long long)h->m_total;
    M.acc = (DevAcc *)h->d_acc.p; M.host_acc = I.host_acc; M.seq = I.seq;
    M.misc = (uint32_t *)h->d_misc.p;
    M.mrun = (double *)h->d_mrun.p;
    M.gsum_next = gs + gt.next;
    M.gdirty_next = gt.dirty_next;
    M.ctl = (IterCtl *)h->d_ctl.p; M.par = h->ctl_par;
    M.thr = I.thr; M.nmax = ds_cap(h); M.dcap2 = h->scene.dcap * h->scene.dcap * (1.0 - 1e-6);
    M.tbox = G.tbox; M.pbox = G.tbox ? (uint32_t *)h->d_pbox.p : nullptr;
    M.popT = nullptr; M.capT = 0; M.cbase_in = nullptr; M.cbase_out = nullptr;
    M.first = 1; M.last = 1;
    if (I.C < I.N) {                    // chunk base / C of several
        const int64_t k = base / I.C;
        unsigned long long *cb = (unsigned long long *)h->d_cbase.p;
        M.popT = h->T.f(0); M.capT = h->T.cap;
        M.cbase_in = cb + (k & 1) * 3; M.cbase_out = cb + ((k & 1) ^ 1) * 3;
        M.first = base == 0 ? 1 : 0;
        M.last = base + nc >= I.N ? 1 : 0;
        if (!M.last) { M.host_acc = nullptr; M.ctl = nullptr; }   // the last chunk publishes the totals
    }
    with_bool(ds != nullptr, [&](auto dsz) {
        hipLaunchKernelGGL(k_stage_move<decltype(dsz)::value>, dim3((unsigned)nt), dim3(LPC_ST_TILE), 0, h->stream, M);
    });
    ledgers_sum(h, I, in, base, nc, LPC_ST_TILE, kSumCulled | kSumRecords);
    // k_shade_stage restored what it read, k_stage_move reset the next launch's words
    h->slots = SlotState{/*clean*/ true, h->emitted.max_ray_len, /*misc_clean*/ true};
    HIPCHK(h, hipGetLastError());
    return 0;
}

// A chunk's per-ray results into the caller's arrays, synchronously (lpc_trace_iterate).
static int copy_per_ray(lpc_handle *h, const IterOut &O, const RaysIn &in, const ShadeOutPtrs &o, int64_t base,
                        int64_t nc)
{
    // the copies below run on the null stream: the shading on h->stream first
    HIPCHK(h, hipStreamSynchronize(h->stream));
    auto pack = [&](float *dst4, const float *x, const float *y, const float *z) -> int {
        hipLaunchKernelGGL(k_pack4, dim3(grid1(nc)), dim3(256), 0, h->stream, nc, x, y, z,
                           (float4 *)h->w_stage.p);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(dst4 + 4 * base, h->w_stage.p, (size_t)nc * 16, hipMemcpyDeviceToHost));
        return 0;
    };
    if (O.origin4) RETIF(pack(O.origin4, in.ox, in.oy, in.oz));
    if (O.dest4) RETIF(pack(O.dest4, o.destx, o.desty, o.destz));
    if (O.pow) HIPCHK(h, hipMemcpy(O.pow + base, o.pw, (size_t)nc * 4, hipMemcpyDeviceToHost));
    if (O.meas) HIPCHK(h, hipMemcpy(O.meas + base, o.meas, (size_t)nc * 4, hipMemcpyDeviceToHost));
    return 0;
}

// One chunk of an iteration with per-ray results: k_shade, then the compaction
// in three kernels (k_count, k_scan, k_scatter), the results taken in between.
static int enqueue_plain_chunk(lpc_handle *h, const IterPlan &I, const IterOut &O, const RaysIn &in, int64_t base,
                               int64_t nc)
{
    const size_t mc = (size_t)h->m_cap;
    float *mf = (float *)h->m_buf.p;
    const ShadeOutPtrs o = shade_ptrs(h, false);
    CompactArgs A;
    A.n = nc; A.nb = (nc + 1023) / 1024; A.o = o;
    A.blk_cnt = (int32_t *)h->w_blk_cnt.p; A.blk_off = (long long *)h->w_blk_off.p;
    A.blk_pow = (double *)h->w_blk_pow.p; A.acc = (DevAcc *)h->d_acc.p;
    A.nR = h->B.out(); A.nT = h->T.out();
    A.direct_t = (I.C >= I.N) ? 1 : 0;                  // one chunk: no refracted staging
    if (A.direct_t) A.nT = A.nR;
    A.mx = mf; A.my = mf + mc; A.mz = mf + 2 * mc; A.mp = mf + 3 * mc;
    A.mm = (int32_t *)(mf + 4 * mc);
    A.host_acc = I.host_acc;
    A.seq = I.seq;
    A.cut = h->led.min_power; A.blk_cc = (uint32_t *)I.L.CS.cc; A.blk_cp = (double *)I.L.CS.cp;
    if (I.L.on.rec()) {                 // k_shade with the fate records, and their sums
        const ShadeArgs SA = shade_args(h, in, nullptr, nc, h->emitted.max_ray_len, h->emitted.ior_env, false);
        with_ku(h->scene.K, [&](auto ku) {
            hipLaunchKernelGGL(k_shade_bud<decltype(ku)::value>, dim3(grid1(nc)), dim3(256), 0, h->stream, SA, I.L.R,
                               I.L.tri, I.L.dest, (int64_t)h->ws_rays);
        });
        HIPCHK(h, hipGetLastError());
        ledgers_sum(h, I, in, base, nc, 1024, kSumRecords);
    } else {
        RETIF(run_shade(h, in, nullptr, nc, h->emitted.max_ray_len, h->emitted.ior_env, false));
    }
    with_bool(I.L.on.cut, [&](auto ct) {
        hipLaunchKernelGGL(k_count<decltype(ct)::value>, dim3((unsigned)A.nb), dim3(256), 0, h->stream, A);
    });
    ledgers_sum(h, I, in, base, nc, 1024, kSumCulled);
    if (O.X) {
        const double hx = h->knobs.host_prof ? host_us() : 0.0;
        RETIF(export_chunk(h, in, o, nc, base, I.N, *O.X));
        if (h->knobs.host_prof) fprintf(stderr, "[lpc host]   export chunk %.1f us\n", host_us() - hx);
    }
    if (O.per_ray()) RETIF(copy_per_ray(h, O, in, o, base, nc));
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, h->stream, A);
    with_bool(I.L.on.cut, [&](auto ct) {
        hipLaunchKernelGGL(k_scatter<decltype(ct)::value>, dim3((unsigned)A.nb), dim3(256), 0, h->stream, A);
    });
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Enqueue one iteration over the current population (host-sized: h->pop.n rays;
// ds != NULL: device-sized, traced single-chunk only).  Host bookkeeping that
// needs no counters (the population's role) happens here; iter_collect the rest.
// thr: the stop threshold a fused iteration's k_stage_move applies when it sizes
// the iteration after it (IterPlan::thr).
static int iter_enqueue(lpc_handle *h, const IterOut &O, const DevSize *ds, double thr, Pending *P)
{
    *P = Pending();
    P->before = h->pop;
    P->slot = h->led.it_done + (ds ? 1 : 0);
    if (h->led.budget) h->led.bud_seen = true;  // (an empty population too: its row is zeros)
    IterPlan I;
    const int64_t N = I.N = ds ? ds->bound : h->pop.n;
    P->n_in = ds ? -1 : N;
    P->ds = ds != nullptr;
    P->n_bound = N;
    if (N == 0) { P->empty = true; return 0; }
    const int64_t C = I.C = std::min(N, chunk_rays(h));
    if (ds && C < N) return set_err(h, LPC_E_STATE, "internal: device-sized iteration over one chunk only");
    I.ds = ds;
    const double hp0 = h->knobs.host_prof ? host_us() : 0.0;
    RETIF(ensure_ws(h, C));
    RETIF(pop_reserve(h, h->B, 2 * N));
    if (!ds) RETIF(pop_reserve(h, h->T, N));
    // measured rows: the iterations still in flight may append up to their populations
    RETIF(ensure_measured(h, h->m_total + h->m_inflight + N));
    RETIF(ledgers_setup(h, &I, P));
    if (h->knobs.host_prof)
        fprintf(stderr, "[lpc host]   buffers %.1f us (m_total %lld inflight %lld m_cap %lld)\n", host_us() - hp0,
                (long long)h->m_total, (long long)h->m_inflight, (long long)h->m_cap);
    h->m_inflight += N;
    IsectIn ii;
    // the counters' reset: device-sized, none (k_stage_move writes every counter);
    // one chunk, it rides on that chunk's slot reset; several, a launch of its own
    ii.acc_reset = !ds && C >= N;
    ii.acc_total = h->m_total;
    if (!ds && C < N)
        hipLaunchKernelGGL(k_acc_init, dim3(1), dim3(64), 0, h->stream, (DevAcc *)h->d_acc.p,
                           (unsigned long long)h->m_total);
    // traced mode: no per-ray export (the population then comes out in its
    // parents' coherence order; measured rays per iteration likewise), shaded and
    // compacted fused (enqueue_fused_chunk)
    const bool traced = !(O.per_ray() || O.next_pow || O.X);
    // the counters come back through the mapped host ring k_scan / k_stage_move
    // write, so the host decides and launches the next iteration while the rows
    // still move (profiling: only the light level, whose events end before)
    const bool early = h->acc_map_dev && (C >= N || traced) && !O.next_pow && (!h->prof.on || h->prof.light);
    ++h->acc_seq;
    P->seq = I.seq = h->acc_seq;
    P->early = early;
    if (traced && C < N) RETIF(dalloc(h, h->d_cbase, 8 * sizeof(unsigned long long)));
    if (ds && !(traced && early)) return set_err(h, LPC_E_STATE, "internal: device-sized iteration off the fused path");
    P->fused = traced;
    P->thr = I.thr = thr;
    // fused: it sums the measured power per measure mesh when they fit (StageArgs::nmp)
    P->mp_fused = traced && h->scene.meas_meshes.size() <= (size_t)LPC_MP_MAX;
    I.host_acc = early ? h->acc_map_dev + P->seq % kAccRing : nullptr;
    // fused: the children's origin box when they may be re-sorted (population >= LPC_RESORT_MIN)
    I.want_box = traced && !ds && 2 * N >= h->knobs.resort_min;
    ii.max_ray_len = h->emitted.max_ray_len; ii.dmax2 = h->pop.dmax2; ii.ds = ds;
    ii.trace = true; ii.traced = traced;
    const bool timed = h->prof.on && !h->prof.light;
    for (int64_t base = 0; base < N; base += C) {
        const int64_t nc = ii.n = std::min(C, N - base);
        ii.rays = (h->pop.init ? h->I : h->A).in(base);
        IsectOut io;
        RETIF(run_intersect(h, ii, &io));
        Event e0, e1;                   // profiling: the chunk's remaining kernels
        if (timed) { e0 = ev_get(h); e1 = ev_get(h); (void)hipEventRecord(e0, h->stream); }
        if (traced) RETIF(enqueue_fused_chunk(h, I, io.traced, io.tmask, base, nc));
        else RETIF(enqueue_plain_chunk(h, I, O, ii.rays, base, nc));
        if (timed) {
            (void)hipEventRecord(e1, h->stream);
            h->prof.ev_rest.emplace_back(std::move(e0), std::move(e1));
        }
    }
    // refracted block after the reflected one (k_append reads the counts on the
    // device), then the counters to the pinned copy: one host sync per iteration
    if (C < N) {
        hipLaunchKernelGGL(k_append, dim3((unsigned)std::min<int64_t>(grid1(N), 8192)), dim3(256), 0, h->stream,
                           h->B.out(), h->T.in(), (const DevAcc *)h->d_acc.p, h->B.cap, h->T.cap);
        HIPCHK(h, hipGetLastError());
    }
    h->ctl_par ^= 1;                    // the next iteration reads the entry this one's k_stage_move writes
    // the children are the next population (their count and max |D|^2 come with iter_collect)
    std::swap(h->A, h->B);
    h->pop = PopState{h->pop.n, h->pop.dmax2, /*init*/ false, traced, /*emitted*/ false, /*pbox_ok*/ I.want_box};
    h->inflight = true;                 // k_stage_move / k_scatter may still run
    return 0;
}

// Read an enqueued iteration's counters (in enqueue order) and finish its host
// bookkeeping.  out_next_pow: the kept children's power (the population after it).
static int iter_collect(lpc_handle *h, const Pending &P, float *out_next_pow, lpc_iter_stats *st)
{
    lpc_iter_stats S;
    memset(&S, 0, sizeof(S));
    S.n_in = P.n_in;
    S.power_nonneg = 1;
    ++h->led.it_done;                   // the ledgers' slot count (an empty iteration's slot stays zero)
    if (P.empty) { if (st) *st = S; return 0; }
    RETIF(ledgers_commit(h, P));
    DevAcc acc;
    const double t_wait = h->knobs.host_prof ? host_us() : 0.0;
    if (P.early) {
        RETIF(wait_mapped_acc(h, P.seq, &acc));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->acc_host, h->d_acc.p, sizeof(DevAcc), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        acc = *h->acc_host;
    }
    h->m_inflight -= P.n_bound;
    if (acc.qerr) return q_failed(h);
    if (h->knobs.host_prof) {
        const double t_got = host_us();
        fprintf(stderr, "[lpc host] n %lld%s  since last %.1f us  wait %.1f us\n", (long long)P.n_in,
                P.ds ? " (device-sized)" : "", t_wait - h->host_last, t_got - t_wait);
        h->host_last = t_got;
    }
    const int64_t nR = (int64_t)acc.nR, nT = (int64_t)acc.nT;
    if (out_next_pow && nR + nT > 0) {   // the population after the swap (iter_enqueue)
        HIPCHK(h, hipMemcpyAsync(out_next_pow, h->A.f(6), (size_t)(nR + nT) * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (h->prof.on) prof_resolve(h);
    h->pop.n = nR + nT;
    h->m_total = (int64_t)acc.m_total;
    // the running per-mesh measured power stays valid while every iteration sums it
    h->mp_valid = h->mp_valid && P.mp_fused;
    if (h->mp_valid) memcpy(h->mp_last, acc.mpow, sizeof(h->mp_last));
    S.n_reflect = nR; S.n_refract = nT; S.n_measured = (int64_t)acc.nM_iter;
    S.power_next = acc.pow_next;
    S.power_nonneg = P.fused ? -1 : (acc.pneg ? 0 : 1);
    float dm2;
    memcpy(&dm2, &acc.dmax2_bits, 4);
    RETIF(check_dcap(h, (double)dm2));
    h->pop.dmax2 = (double)dm2;                 // the next population's max |D|^2 (float, see run_intersect)
    if (st) *st = S;
    return 0;
}

// A sharded trace's dropped speculative iteration may have run non-empty: its
// k_stage_move added its measured power to the trace's running sums on the
// device; they go back to the last read iteration's (the host copy).  Its
// measured rows lie past m_total and its children in the scratch population,
// both ignored.
static int restore_mrun(lpc_handle *h)
{
    if (!h->mp_valid || !h->d_mrun.p) return 0;
    // rare (a misprediction at the trace's end): after the dropped iteration's
    // kernels, a synchronous copy from the handle's host copy
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->d_mrun.p, h->mp_last, sizeof(h->mp_last), hipMemcpyHostToDevice));
    return 0;
}

// A speculative iteration the trace did not need (it ran empty on the device:
// IterCtl said 0): the population roles go back to before its enqueue.
static void iter_discard(lpc_handle *h, const Pending &P)
{
    h->m_inflight -= P.n_bound;
    if (P.empty) return;
    std::swap(h->A, h->B);
    // the size and max |D|^2 are iter_collect's, not the enqueue's: they stay
    const PopState now = h->pop;
    h->pop = P.before;
    h->pop.n = now.n; h->pop.dmax2 = now.dmax2;
}

int lpc_trace_iterate(lpc_handle *h, float *out_origin4, float *out_dest4, float *out_pow,
                      int32_t *out_meas, float *out_next_pow, lpc_iter_stats *st)
{
    const double t_enter = h && h->knobs.host_prof ? host_us() : 0.0;
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(need_rays(h, "trace_iterate"));
    HIPCHK(h, hipSetDevice(h->device));
    Pending P;
    RETIF(iter_enqueue(h, IterOut{out_origin4, out_dest4, out_pow, out_meas, out_next_pow}, nullptr, -INFINITY, &P));
    if (h->knobs.host_prof && !P.empty)
        fprintf(stderr, "[lpc host] n %lld  launch %.1f us\n", (long long)P.n_in, host_us() - t_enter);
    return iter_collect(h, P, out_next_pow, st);
}

int lpc_trace_iterate_export(lpc_handle *h, void *host, int32_t flags, lpc_iter_stats *st)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (!host) return set_err(h, LPC_E_ARG, "trace_iterate_export: null host block");
    RETIF(need_rays(h, "trace_iterate_export"));
    HIPCHK(h, hipSetDevice(h->device));
    const double t_enter = h->knobs.host_prof ? host_us() : 0.0;
    const ExportSpec X{(char *)host, (flags & 1) ? 1 : 0};
    IterOut O;
    O.X = &X;
    Pending P;
    RETIF(iter_enqueue(h, O, nullptr, -INFINITY, &P));
    if (h->knobs.host_prof && !P.empty)
        fprintf(stderr, "[lpc host] n %lld  export launch %.1f us\n", (long long)P.n_in, host_us() - t_enter);
    return iter_collect(h, P, nullptr, st);
}

int lpc_trace_population_power(lpc_handle *h, float *out)
{
    if (!h || !out) return set_err(h, LPC_E_ARG, "null argument");
    RETIF(settle(h));
    if (h->pop.n > 0) {
        const Pop &P = h->pop.init ? h->I : h->A;
        HIPCHK(h, hipMemcpy(out, P.f(6), (size_t)h->pop.n * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

int lpc_host_alloc(size_t bytes, void **out)
{
    if (!out) return set_err(nullptr, LPC_E_ARG, "host_alloc: null output");
    *out = nullptr;
    const hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(nullptr, LPC_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return 0;
}

int lpc_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
    return 0;
}

int lpc_host_seq_sum_f32(const float *x, int64_t n, float *out)
{
    if (!out || (n > 0 && !x) || n < 0) return set_err(nullptr, LPC_E_ARG, "host_seq_sum_f32: bad argument");
    // np.add.accumulate's order: x[0], then + x[1], ... (no reassociation: the
    // build has no fast-math; the adds form one dependent chain)
    float s = n > 0 ? x[0] : 0.0f;
    for (int64_t i = 1; i < n; ++i) s += x[i];
    *out = s;
    return 0;
}

// May the iteration after the one in flight (population <= bound rays, chained
// traced) be enqueued device-sized?  Single chunk, fused compaction, mapped
// counters, root-item path, no per-kernel profiling.  A sharded trace (all-reduce
// hook) speculates too: the device then stops only on an empty local population,
// and the host drops the iteration when the ranks' sums end the trace.
static bool ds_ok(const lpc_handle *h, int64_t bound)
{
    return h->knobs.spec && h->acc_map_dev && (!h->prof.on || h->prof.light) && bound > 0 && bound <= chunk_rays(h) &&
           bound < h->knobs.resort_min && (bound + 63) / 64 <= (int64_t)LPC_Q_MAX_PACKETS;
}

// The trace loop (iterative_tracer.py:383-391).  With speculation (LPC_SPEC, and
// a previous trace of the same first population, limit and threshold that
// reached the next iteration), iteration i + 1 is enqueued device-sized
// (IterCtl: its size and the stop rule evaluated by iteration i's k_stage_move)
// before iteration i's counters are read, so the GPU never waits for the host
// between iterations.  The results are the same bits: the device applies the
// host's rules; an iteration the trace turns out not to need runs empty and is
// dropped (iter_discard); a Dcap overflow (records rebuilt) re-runs it host-sized.
static int trace_run(lpc_handle *h, int32_t max_iter, double power_threshold, lpc_iter_stats *per_iter,
                     int32_t *n_iter, int64_t *measured_count, double *mesh_power, int32_t mesh_power_cap,
                     bool wait)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (!n_iter || (max_iter > 0 && !per_iter)) return set_err(h, LPC_E_ARG, "trace_run: null output");
    // mesh_power receives one double per mesh of the CURRENT scene: a buffer sized
    // for an earlier scene with fewer meshes is refused, not overrun
    if (mesh_power && mesh_power_cap < h->scene.K)
        return set_err(h, LPC_E_ARG, "trace: mesh_power capacity below the scene's mesh count");
    RETIF(need_rays(h, "trace_run"));
    if (h->knobs.host_prof)                           // the caller's time between traces
        fprintf(stderr, "[lpc host] trace enter  since last %.1f us\n", host_us() - h->host_last);
    HIPCHK(h, hipSetDevice(h->device));
    *n_iter = 0;
    h->gstats.clear();
    // the prediction: the last trace from emitted rays with this iteration limit
    // (which iterations it reached, populations relative to the first)
    const int64_t n0 = h->pop.emitted ? h->pop.n : -1;
    const bool hist_ok = n0 > 0 && h->hist_iter == max_iter && !h->hist_r.empty();
    h->dcap_rebuilt = false;
    std::vector<int64_t> seen;
    // the device's stop rule for speculative iterations (k_stage_move, local_thr
    // below): the threshold on this device's own power left -- or, in a sharded
    // trace, none: the power left is a sum over all ranks, only the host sees it
    // after the exchange, and a speculative iteration the ranks' sums end is dropped;
    // sharded: a conservative local rule.  The device may stop the trace only when
    // the ranks' sum is certain to fall below the threshold: with passive
    // materials and non-negative powers a population's power never grows, so the
    // other ranks' power left after the last exchanged iteration j bounds theirs
    // at every later iteration (slack for the float32 children sums), and this
    // rank's power below threshold - that bound ends the global trace too.
    const Emitted &E = h->emitted;
    const bool mono = h->xchg && h->scene.mat_passive && E.pow_nonneg && E.ior_env > 0.0f && std::isfinite(E.ior_env);
    double others = INFINITY;           // upper bound of the other ranks' power left (last exchange)
    int32_t others_it = -1;
    auto local_thr = [&](int32_t it) {  // k_stage_move's stop threshold of iteration `it`
        if (!h->xchg) return power_threshold;
        if (!mono || others_it < 0 || !(others < INFINITY)) return -(double)INFINITY;
        return power_threshold - others * (1.0 + 1e-5 * (double)(it - others_it + 1));
    };
    int rc = 0;
    bool exchanged = false;             // rc came from the exchange itself (no poison owed)
    int32_t post_fail = -1;             // failed after this iteration's exchange: the shape the peers wait in next
    Pending cur, nxt;
    bool have_cur = false, have_nxt = false;
    for (int32_t i = 0; i < max_iter; ++i) {
        if (!have_cur) {
            if ((rc = iter_enqueue(h, IterOut(), nullptr, local_thr(i), &cur))) break;
            have_cur = true;
        }
        // iteration i + 1, device-sized, while iteration i runs (its population is
        // known: host-sized, or the kept children of iteration i - 1)
        if (hist_ok && i + 1 < max_iter && (int64_t)h->hist_r.size() > i + 1 && cur.fused && !cur.empty &&
            cur.n_in > 0) {
            // its bound: all children of the current population, capped at
            // ds_cap (more kept children: it runs empty and is re-run host-sized)
            const int64_t bound = std::min<int64_t>(2 * cur.n_in, ds_cap(h));
            const int64_t pred_n = (int64_t)llround(h->hist_r[(size_t)i + 1] * (double)n0);
            if (pred_n <= bound && ds_ok(h, bound)) {
                IterCtl *ctl = (IterCtl *)h->d_ctl.p;
                DevSize D;
                D.nd = &ctl->n[h->ctl_par];
                D.dm2 = &ctl->dm2[h->ctl_par];
                D.pred = std::max<int64_t>(1, std::min(pred_n, bound));
                D.bound = bound;
                if ((rc = iter_enqueue(h, IterOut(), &D, local_thr(i + 1), &nxt))) break;
                have_nxt = true;
            }
        }
        lpc_iter_stats S;
        const double cur_thr = cur.thr;     // the stop rule cur's k_stage_move sized nxt with
        rc = iter_collect(h, cur, nullptr, &S);
        have_cur = false;
        if (rc) break;
        per_iter[i] = S;
        *n_iter = i + 1;
        seen.push_back(S.n_in);
        // sharded trace: every rank decides on the sums over all ranks (the
        // identical bits everywhere), so all stop at the iteration a single
        // device would (iterative_tracer.py:383-391)
        lpc_iter_stats G = S;
        if (h->xchg && (rc = xchg_stats(h, S, &G))) { exchanged = true; break; }
        h->gstats.push_back(G);
        if (h->xchg) {
            others = std::max(0.0, G.power_next - S.power_next) * (1.0 + 1e-9);
            others_it = i;
        }
        const bool stop = G.power_next < power_threshold || G.n_reflect + G.n_refract == 0;   // :383, :389
        if (have_nxt) {
            const bool rebuilt = h->dcap_rebuilt;
            h->dcap_rebuilt = false;
            if (stop || rebuilt || i + 1 >= max_iter) {
                // not part of the trace: it ran empty on the device (its IterCtl
                // size was 0) -- or, sharded, it may have run on this rank's kept
                // children when the ranks' sums stopped the trace; after a Dcap
                // rebuild its measured power must not count either
                iter_discard(h, nxt);
                have_nxt = false;
                if ((h->xchg || rebuilt) && (rc = restore_mrun(h))) {
                    // this iteration's exchange is done: the peers wait next in
                    // the trace-end sums (stop) or the next iteration's stats
                    post_fail = stop ? ((measured_count || mesh_power) ? h->scene.K + 2 : 0) : LPC_XCHG_STATS;
                    break;
                }
            } else if (S.n_reflect + S.n_refract > nxt.n_bound || S.power_next < cur_thr) {
                // more children than it was sized for, or this device's stop rule
                // fired where the trace goes on (a sharded rank's local bound,
                // should its premise fail): it ran empty on the device; the next
                // pass of the loop runs the iteration host-sized
                iter_discard(h, nxt);
                have_nxt = false;
                if (h->xchg && (rc = restore_mrun(h))) { post_fail = LPC_XCHG_STATS; break; }
            } else {
                nxt.n_in = S.n_reflect + S.n_refract;           // this rank's population
                cur = nxt;
                have_cur = true;
                have_nxt = false;
            }
        }
        if (stop) break;
    }
    if (have_nxt) iter_discard(h, nxt);
    if (have_cur) {                                         // an error with one still queued
        (void)hipStreamSynchronize(h->stream);
        iter_discard(h, cur);
    }
    if (rc && !exchanged) {
        if (post_fail < 0) xchg_poison(h, LPC_XCHG_STATS);               // the peers wait in this iteration's exchange
        else if (post_fail > 0) xchg_poison(h, post_fail);
    }
    RETIF(rc);
    // this trace's populations (relative to the first) predict the next trace's
    if (n0 > 0) {
        h->hist_r.clear();
        for (int64_t v : seen) h->hist_r.push_back((double)v / (double)n0);
        h->hist_iter = max_iter;
    }
    if (measured_count || mesh_power) {                     // the trace's aggregates, same call
        // [failure flag, per-mesh power (K), measured count]
        int64_t c = 0;
        std::vector<double> mp((size_t)h->scene.K + 2, 0.0);
        if ((rc = lpc_trace_measured(h, &c, mp.data() + 1, h->scene.K))) {
            xchg_poison(h, h->scene.K + 2);
            return rc;
        }
        if (h->xchg) {                                      // trace-end sums over the ranks
            mp[(size_t)h->scene.K + 1] = (double)c;
            if (h->xchg(h->xchg_ctx, mp.data(), h->scene.K + 2) != 0)
                return set_err(h, LPC_E_STATE, "trace: all-reduce hook failed");
            if (mp[0] != 0.0) return set_err(h, LPC_E_STATE, "trace: a peer rank failed (failure flag in the trace-end sums)");
            c = (int64_t)mp[(size_t)h->scene.K + 1];
        }
        if (measured_count) *measured_count = c;
        if (mesh_power) memcpy(mesh_power, mp.data() + 1, (size_t)h->scene.K * 8);
    }
    if (wait) RETIF(settle(h));                             // the trace's last kernels too
    if (h->knobs.host_prof) {
        const double t = host_us();
        fprintf(stderr, "[lpc host] trace leave  since last %.1f us\n", t - h->host_last);
        h->host_last = t;
    }
    return 0;
}

static int mesh_power(lpc_handle *h, double *out)
{
    for (int32_t j = 0; j < h->scene.K; ++j) out[j] = 0.0;
    if (h->m_total == 0) return 0;
    if (h->mp_valid && h->scene.meas_meshes.size() <= (size_t)LPC_MP_MAX) {  // summed per tile by the traced iterations
        for (size_t m = 0; m < h->scene.meas_meshes.size(); ++m) out[h->scene.meas_meshes[m]] = h->mp_last[m];
        return 0;
    }
    const int64_t nb = (h->m_total + LPC_MSUM_TILE - 1) / LPC_MSUM_TILE;
    RETIF(dalloc(h, h->d_tmp, (size_t)nb * 8));
    std::vector<double> part((size_t)nb);
    const size_t mc = (size_t)h->m_cap;
    const float *mf = (const float *)h->m_buf.p;
    for (int32_t j : h->scene.meas_meshes) {
        hipLaunchKernelGGL(k_mesh_sum, dim3((unsigned)nb), dim3(256), 0, h->stream, h->m_total,
                           mf + 3 * mc, (const int32_t *)(mf + 4 * mc), j, (double *)h->d_tmp.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(part.data(), h->d_tmp.p, (size_t)nb * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        double s = 0.0;
        for (double v : part) s += v;
        out[j] = s;
    }
    return 0;
}

int lpc_trace_measured(lpc_handle *h, int64_t *count, double *mesh_pow, int32_t mesh_pow_cap)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (mesh_pow && mesh_pow_cap < h->scene.K)
        return set_err(h, LPC_E_ARG, "trace_measured: mesh_power capacity below the scene's mesh count");
    HIPCHK(h, hipSetDevice(h->device));
    if (count) *count = h->m_total;
    if (mesh_pow) RETIF(mesh_power(h, mesh_pow));
    return 0;
}

int lpc_trace_fetch_measured(lpc_handle *h, float *pos4, float *pow, int32_t *mesh)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t n = h->m_total;
    if (n == 0) return 0;
    const size_t mc = (size_t)h->m_cap;
    const float *mf = (const float *)h->m_buf.p;
    if (pos4) {
        RETIF(dalloc(h, h->w_stage, (size_t)n * 16));
        hipLaunchKernelGGL(k_pack4, dim3(grid1(n)), dim3(256), 0, h->stream, n, mf, mf + mc,
                           mf + 2 * mc, (float4 *)h->w_stage.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(pos4, h->w_stage.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    }
    if (pow) HIPCHK(h, hipMemcpy(pow, mf + 3 * mc, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (mesh) HIPCHK(h, hipMemcpy(mesh, mf + 4 * mc, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int lpc_project_hist(lpc_handle *h, int mode, int64_t n, const float *pos4, const float *pwr,
                     const float *rot4, const float *pivot4, const double *xedges, int nx,
                     const double *yedges, int ny, double weight_div, double *H, float *x,
                     float *y, float *pwr_cor)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    if ((mode != 0 && mode != 1) || nx <= 0 || ny <= 0 || !rot4 || !pivot4 || !xedges || !yedges || !H)
        return set_err(h, LPC_E_ARG, "project_hist: bad argument");
    if (pos4 && !pwr) return set_err(h, LPC_E_ARG, "project_hist: pwr is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos4) n = h->m_total;
    if (n < 0) return set_err(h, LPC_E_ARG, "project_hist: negative n");
    // device scratch: [rot 16 f | piv 4 f | xe | ye | H | (pos4, pwr) | (x, y, pc)]
    const size_t o_rot = 0, o_xe = 128, o_ye = o_xe + (size_t)(nx + 1) * 8;
    const size_t o_H = (o_ye + (size_t)(ny + 1) * 8 + 255) / 256 * 256;
    const size_t o_in = (o_H + (size_t)nx * ny * 8 + 255) / 256 * 256;
    const size_t in_bytes = pos4 ? (size_t)n * 20 : 0;
    const size_t o_out = (o_in + in_bytes + 255) / 256 * 256;
    const size_t out_bytes = x ? (size_t)n * 12 : 0;
    RETIF(dalloc(h, h->d_tmp, o_out + out_bytes + 16));
    char *d = (char *)h->d_tmp.p;
    float rp[20];
    memcpy(rp, rot4, 16 * 4);
    memcpy(rp + 16, pivot4, 4 * 4);
    HIPCHK(h, hipMemcpy(d + o_rot, rp, sizeof(rp), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + o_xe, xedges, (size_t)(nx + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + o_ye, yedges, (size_t)(ny + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemsetAsync(d + o_H, 0, (size_t)nx * ny * 8, h->stream));
    ProjArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.mode = mode;
    if (pos4) {
        HIPCHK(h, hipMemcpy(d + o_in, pos4, (size_t)n * 16, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d + o_in + (size_t)n * 16, pwr, (size_t)n * 4, hipMemcpyHostToDevice));
        A.pos4 = (const float4 *)(d + o_in);
        A.pwr = (const float *)(d + o_in + (size_t)n * 16);
    } else {
        const size_t mc = (size_t)h->m_cap;
        const float *mf = (const float *)h->m_buf.p;
        A.px = mf; A.py = mf + mc; A.pz = mf + 2 * mc; A.pwr = mf + 3 * mc;
    }
    A.rot = (const float *)(d + o_rot);
    A.piv = (const float *)(d + o_rot) + 16;
    if (x) { A.x = (float *)(d + o_out); A.y = A.x + n; A.pc = A.y + n; }
    A.xe = (const double *)(d + o_xe); A.ye = (const double *)(d + o_ye);
    A.nx = nx; A.ny = ny; A.div = weight_div; A.H = (double *)(d + o_H);
    if (n > 0) {
        hipLaunchKernelGGL(k_project_hist, dim3(grid1(n)), dim3(256), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(H, d + o_H, (size_t)nx * ny * 8, hipMemcpyDeviceToHost));
    if (x && n > 0) {
        HIPCHK(h, hipMemcpy(x, A.x, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (y) HIPCHK(h, hipMemcpy(y, A.y, (size_t)n * 4, hipMemcpyDeviceToHost));
        if (pwr_cor) HIPCHK(h, hipMemcpy(pwr_cor, A.pc, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    return 0;
}

// One-pass map (k_map_hist): all rotations of every point binned on the device,
// only the histogram (and its statistics) copied back.  With profiling on
// (lpc_prof_enable) the launch's own start / stop timestamps go to kernel_ms.
int lpc_map_hist(lpc_handle *h, int mode, int64_t n, const float *pos4, const float *pwr,
                 const float *rot4, int32_t n_rot, const float *pivot4, const double *xedges, int nx,
                 const double *yedges, int ny, double weight_div, double *H, int64_t *count, double *H2)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    if (mode < 0 || mode > 2) return set_err(h, LPC_E_ARG, "map_hist: mode outside 0..2");
    if (n_rot < 1) return set_err(h, LPC_E_ARG, "map_hist: n_rot < 1");
    if (nx < 1 || ny < 1) return set_err(h, LPC_E_ARG, "map_hist: nx or ny < 1");
    if (!xedges || !yedges || !H) return set_err(h, LPC_E_ARG, "map_hist: edges or H is NULL");
    if (pos4 && !pwr) return set_err(h, LPC_E_ARG, "map_hist: pwr is NULL");
    if (pos4 && n < 0) return set_err(h, LPC_E_ARG, "map_hist: negative n");
    if ((int64_t)nx * ny > (int64_t)INT32_MAX) return set_err(h, LPC_E_ARG, "map_hist: nx * ny beyond 2^31 - 1 bins");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos4) n = h->m_total;
    const bool stats = count || H2;
    const size_t nb = (size_t)nx * ny, nr = rot4 ? (size_t)n_rot : 1;
    // device scratch: [rot n_rot x 16 f | piv 4 f | xe | ye | H | H2 | C | (pos4, pwr)]
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_piv = nr * 64, o_xe = up(o_piv + 16), o_ye = o_xe + (size_t)(nx + 1) * 8;
    const size_t o_H = up(o_ye + (size_t)(ny + 1) * 8);
    const size_t o_in = up(o_H + nb * 8 * (stats ? 3 : 1));
    RETIF(dalloc(h, h->d_tmp, o_in + (pos4 ? (size_t)n * 20 : 0) + 16));
    char *d = (char *)h->d_tmp.p;
    static const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0};
    static const float zero4[4] = {0, 0, 0, 0};
    HIPCHK(h, hipMemcpy(d, rot4 ? rot4 : eye, nr * 64, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + o_piv, pivot4 ? pivot4 : zero4, 16, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + o_xe, xedges, (size_t)(nx + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + o_ye, yedges, (size_t)(ny + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemsetAsync(d + o_H, 0, nb * 8 * (stats ? 3 : 1), h->stream));
    MapArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.mode = mode;
    A.ident = mode == 2 && !rot4;
    if (pos4) {
        if (n > 0) {
            HIPCHK(h, hipMemcpy(d + o_in, pos4, (size_t)n * 16, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d + o_in + (size_t)n * 16, pwr, (size_t)n * 4, hipMemcpyHostToDevice));
        }
        A.pos4 = (const float4 *)(d + o_in);
        A.pwr = (const float *)(d + o_in + (size_t)n * 16);
    } else {
        const size_t mc = (size_t)h->m_cap;
        const float *mf = (const float *)h->m_buf.p;
        A.px = mf; A.py = mf + mc; A.pz = mf + 2 * mc; A.pwr = mf + 3 * mc;
    }
    A.rot = (const float *)d; A.piv = (const float *)(d + o_piv); A.n_rot = (int)nr;
    A.xe = (const double *)(d + o_xe); A.ye = (const double *)(d + o_ye);
    A.nx = nx; A.ny = ny; A.div = weight_div;
    A.H = (double *)(d + o_H);
    if (stats) { A.H2 = A.H + nb; A.C = (unsigned long long *)(A.H2 + nb); }
    if (n > 0) {
        // the LDS histogram: a block holds cap_bins bins (20 B each with the statistics,
        // 4 B of padding), a larger map goes in up to map_slices slices, each a sweep
        // of its own over the points; the uint32 counts of a block cannot wrap
        const bool edges_lds = (size_t)nx + ny + 2 <= LPC_MAP_EDGES;
        const size_t cap_bins = (LPC_MAP_HIST_BYTES - 4) / (stats ? 20 : 8);
        const size_t slices = (nb + cap_bins - 1) / cap_bins;
        const bool hist_lds = h->knobs.map_slices > 0 && edges_lds && slices <= (size_t)h->knobs.map_slices &&
                              (double)n * (double)nr < 4.0e9;
        const int path = hist_lds ? 2 : edges_lds ? 1 : 0;
        const int bs = path == 2 ? 1024 : 256;
        A.slice_bins = (int)((nb + slices - 1) / slices);
        const unsigned gy = path == 2 ? (unsigned)((nb + A.slice_bins - 1) / A.slice_bins) : 1u;
        const int64_t cap = path == 2 ? std::max<int64_t>(1, std::max(h->cus, 1) / (int64_t)gy)
                                      : (int64_t)std::max(h->cus, 1) * h->knobs.map_per_cu;
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + bs - 1) / bs, cap));
        Event k0, k1;
        const bool timed = h->prof.on && !h->prof.light;    // (light: k_rootwalk's events only)
        if (timed) { k0 = ev_get(h); k1 = ev_get(h); }
        auto launch = [&](auto pt, auto st) {
            hipExtLaunchKernelGGL((k_map_hist<decltype(pt)::value, decltype(st)::value>), dim3(grid, gy), dim3(bs), 0,
                                  h->stream, k0, k1, 0, A);
        };
        with_bool(stats, [&](auto st) {
            if (path == 2) launch(std::integral_constant<int, 2>{}, st);
            else if (path == 1) launch(std::integral_constant<int, 1>{}, st);
            else launch(std::integral_constant<int, 0>{}, st);
        });
        HIPCHK(h, hipGetLastError());
        if (timed) h->prof.ev_kern.emplace_back(std::move(k0), std::move(k1));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(H, A.H, nb * 8, hipMemcpyDeviceToHost));
    if (H2) HIPCHK(h, hipMemcpy(H2, A.H2, nb * 8, hipMemcpyDeviceToHost));
    if (count) HIPCHK(h, hipMemcpy(count, A.C, nb * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- elevation analyses (iterative_tracer.py:420-501) -------------------------
// Every lpc_elev_* entry point goes: NULL-handle check, settle, its own argument
// checks, then elev_begin: the points (host points uploaded behind `head` bytes
// of pass scratch in d_tmp, or the measured record) and the pole.  *scratch = the
// head region (256-B aligned).
static int elev_begin(lpc_handle *h, const char *who, int64_t &n, const float *pos4, const float *pwr,
                      const double *pole, size_t head, ElevIn &in, char **scratch)
{
    if (!pole) return set_err(h, LPC_E_ARG, std::string(who) + ": pole is NULL");
    if (pos4 && !pwr) return set_err(h, LPC_E_ARG, std::string(who) + ": pwr is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    if (!pos4) n = h->m_total;
    if (n < 0) return set_err(h, LPC_E_ARG, std::string(who) + ": negative n");
    head = (head + 255) / 256 * 256;
    RETIF(dalloc(h, h->d_tmp, head + (pos4 ? (size_t)n * 20 : 0) + 16));
    char *d = (char *)h->d_tmp.p;
    memset(&in, 0, sizeof(in));
    in.n = n;
    if (pos4) {
        if (n > 0) {
            HIPCHK(h, hipMemcpy(d + head, pos4, (size_t)n * 16, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d + head + (size_t)n * 16, pwr, (size_t)n * 4, hipMemcpyHostToDevice));
        }
        in.pos4 = (const float4 *)(d + head);
        in.pwr = (const float *)(d + head + (size_t)n * 16);
    } else {
        const size_t mc = (size_t)h->m_cap;
        const float *mf = (const float *)h->m_buf.p;
        in.px = mf; in.py = mf + mc; in.pz = mf + 2 * mc; in.pwr = mf + 3 * mc;
    }
    for (int k = 0; k < 4; ++k) in.pole[k] = pole[k];
    *scratch = d;
    return 0;
}
// Grid of the grid-stride elevation kernels: enough blocks to fill the GPU
// (per_cu blocks per CU), never more than the rows.
static inline unsigned elev_grid(const lpc_handle *h, int64_t n, int per_cu)
{
    const int64_t cap = (int64_t)std::max(h->cus, 1) * per_cu;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
}
static inline double bits_to_double(unsigned long long b)
{
    double v;
    memcpy(&v, &b, 8);
    return v;
}

int lpc_elev_scan(lpc_handle *h, int64_t n, const float *pos4, const float *pwr, const double *pole,
                  lpc_elev_summary *out)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    if (!out) return set_err(h, LPC_E_ARG, "elev_scan: out is NULL");
    ElevIn in;
    char *d = nullptr;
    RETIF(elev_begin(h, "elev_scan", n, pos4, pwr, pole, sizeof(ElevScanOut), in, &d));
    ElevScanOut z;
    memset(&z, 0, sizeof(z));
    z.emin_bits = ~0ull;
    HIPCHK(h, hipMemcpy(d, &z, sizeof(z), hipMemcpyHostToDevice));
    if (n > 0) {
        hipLaunchKernelGGL(k_elev_scan, dim3(elev_grid(h, n, 8)), dim3(256), 0, h->stream, in, (ElevScanOut *)d);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&z, d, sizeof(z), hipMemcpyDeviceToHost));
    out->n_valid = (int64_t)z.n_valid;
    out->n_invalid = (int64_t)z.n_invalid;
    out->n_negative = (int64_t)z.n_negative;
    out->e_min = z.n_valid ? bits_to_double(z.emin_bits) : NAN;
    out->e_max = z.n_valid ? bits_to_double(z.emax_bits) : NAN;
    out->total_power = z.total;
    return 0;
}

int lpc_elev_hist(lpc_handle *h, int64_t n, const float *pos4, const float *pwr, const double *pole,
                  const double *edges, int nbins, double *H, double *elev_out)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // h->m_total below is the finished trace's
    if (nbins <= 0 || !edges || !H) return set_err(h, LPC_E_ARG, "elev_hist: bad argument");
    ElevIn in;
    char *d = nullptr;
    // scratch: [edges | H | elev_out (one double per point: n, or the record's length)]
    const int64_t n_out = elev_out ? (pos4 ? n : (int64_t)h->m_total) : 0;
    const size_t o_H = ((size_t)(nbins + 1) * 8 + 255) / 256 * 256;
    const size_t o_e = (o_H + (size_t)nbins * 8 + 255) / 256 * 256;
    RETIF(elev_begin(h, "elev_hist", n, pos4, pwr, pole, o_e + (size_t)std::max<int64_t>(n_out, 0) * 8, in, &d));
    HIPCHK(h, hipMemcpy(d, edges, (size_t)(nbins + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemsetAsync(d + o_H, 0, (size_t)nbins * 8, h->stream));
    ElevHistArgs A;
    A.in = in;
    A.edges = (const double *)d;
    A.nbins = nbins;
    A.H = (double *)(d + o_H);
    A.elev_out = elev_out ? (double *)(d + o_e) : nullptr;
    if (n > 0) {
        with_bool(nbins <= LPC_ELEV_LDS_BINS, [&](auto lds) {
            hipLaunchKernelGGL(k_elev_hist<decltype(lds)::value>, dim3(elev_grid(h, n, 8)), dim3(256), 0, h->stream, A);
        });
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(H, d + o_H, (size_t)nbins * 8, hipMemcpyDeviceToHost));
    if (elev_out && n > 0) HIPCHK(h, hipMemcpy(elev_out, d + o_e, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

int lpc_elev_digit_pass(lpc_handle *h, int64_t n, const float *pos4, const float *pwr, const double *pole,
                        uint64_t prefix, int shift, int bits, double *bin_pow, int64_t *bin_cnt,
                        uint64_t *bin_maxkey)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));
    if (bits < 1 || bits > 12 || shift < 0 || shift + bits > 64 || !bin_pow || !bin_cnt || !bin_maxkey)
        return set_err(h, LPC_E_ARG, "elev_digit_pass: bad argument (1 <= bits <= 12, 0 <= shift, shift + bits <= 64)");
    ElevIn in;
    char *d = nullptr;
    const size_t nb = (size_t)1 << bits;
    RETIF(elev_begin(h, "elev_digit_pass", n, pos4, pwr, pole, nb * 24, in, &d));
    HIPCHK(h, hipMemsetAsync(d, 0, nb * 24, h->stream));
    ElevDigitArgs A;
    A.in = in;
    A.all = shift + bits == 64;
    A.prefix = A.all ? 0ull : (unsigned long long)prefix;
    A.shift = shift;
    A.bits = bits;
    A.bin_pow = (double *)d;
    A.bin_cnt = (unsigned long long *)(d + nb * 8);
    A.bin_maxkey = (unsigned long long *)(d + nb * 16);
    if (n > 0) {
        if (bits <= 11)
            hipLaunchKernelGGL(k_elev_digit<2048>, dim3(elev_grid(h, n, 4)), dim3(256), 0, h->stream, A);
        else
            hipLaunchKernelGGL(k_elev_digit<4096>, dim3(elev_grid(h, n, 2)), dim3(256), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(bin_pow, d, nb * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(bin_cnt, d + nb * 8, nb * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(bin_maxkey, d + nb * 16, nb * 8, hipMemcpyDeviceToHost));
    return 0;
}

int lpc_elev_power_below(lpc_handle *h, int64_t n, const float *pos4, const float *pwr, const double *pole,
                         double thr, int inclusive, double *power, int64_t *count, double *e_max)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));
    ElevIn in;
    char *d = nullptr;
    RETIF(elev_begin(h, "elev_power_below", n, pos4, pwr, pole, sizeof(ElevBelowOut), in, &d));
    HIPCHK(h, hipMemsetAsync(d, 0, sizeof(ElevBelowOut), h->stream));
    ElevBelowArgs A;
    A.in = in;
    A.thr = thr;
    A.inclusive = inclusive != 0;
    A.out = (ElevBelowOut *)d;
    if (n > 0) {
        hipLaunchKernelGGL(k_elev_below, dim3(elev_grid(h, n, 8)), dim3(256), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
    }
    ElevBelowOut r;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&r, d, sizeof(r), hipMemcpyDeviceToHost));
    if (power) *power = r.power;
    if (count) *count = (int64_t)r.count;
    if (e_max) *e_max = r.count ? bits_to_double(r.emax_bits) : NAN;
    return 0;
}

int lpc_filter_eval(lpc_handle *h, int64_t n, const float *origin3, const float *dir3, const float *rec5,
                    int mode, float *out_d)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (n < 0 || mode < 0 || mode > 3 || (n > 0 && (!origin3 || !dir3 || !rec5 || !out_d)))
        return set_err(h, LPC_E_ARG, "filter_eval: bad argument");
    RETIF(settle(h));
    HIPCHK(h, hipSetDevice(h->device));
    if (n == 0) return 0;
    RETIF(dalloc(h, h->d_tmp, (size_t)n * 48));
    float *dO = (float *)h->d_tmp.p, *dD = dO + 3 * n, *dR = dD + 3 * n, *dOut = dR + 5 * n;
    HIPCHK(h, hipMemcpy(dO, origin3, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(dD, dir3, (size_t)n * 12, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(dR, rec5, (size_t)n * 20, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_filter_eval, dim3(grid1(n)), dim3(256), 0, h->stream, n, (const float *)dO,
                       (const float *)dD, (const float *)dR, mode, dOut);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out_d, dOut, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int lpc_prof_enable(lpc_handle *h, int on)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    h->prof.every = std::max(1, on >> 8);           // 4 + 256 k: light, every k-th walk launch
    on &= 0xff;
    h->prof.seq = 0;
    h->prof.on = on != 0;
    h->prof.stats = on == 2;
    h->prof.light = on == 4;                        // k_rootwalk events only (bench timed region)
    if (h->prof.stats && !h->prof.d_stats.p) {
        RETIF(dalloc(h, h->prof.d_stats, LPC_STATS_WORDS * 8));
        HIPCHK(h, hipMemset(h->prof.d_stats.p, 0, LPC_STATS_WORDS * 8));
    }
    return 0;
}

int lpc_prof_read(lpc_handle *h, lpc_prof *out, int reset)
{
    if (!h || !out) return set_err(h, LPC_E_ARG, "null argument");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    (void)hipStreamSynchronize(h->stream);
    prof_resolve(h);
    out->intersect_ms = h->prof.isect_ms;
    out->kernel_ms = h->prof.kern_ms;
    out->shade_ms = h->prof.rest_ms;
    out->intersect_launches = h->prof.launches;
    out->xchg_us = h->xchg_us;
    out->xchg_calls = h->xchg_calls;
    out->pairs = h->prof.pairs;
    std::vector<unsigned long long> st(LPC_STATS_WORDS, 0ull);
    if (h->prof.d_stats.p) HIPCHK(h, hipMemcpy(st.data(), h->prof.d_stats.p, LPC_STATS_WORDS * 8, hipMemcpyDeviceToHost));
    out->node_visits = (int64_t)st[0];
    out->group_tests = (int64_t)st[1];
    out->wave_traversals = (int64_t)st[2];
    out->exact_tests = (int64_t)st[3];
    for (int b = 0; b < 24; ++b) out->wave_hist[b] = (int64_t)st[LPC_STATS_HIST + b];
    out->tail_waves = (int64_t)st[4]; out->tail_nodes = (int64_t)st[5];
    out->tail_spread_urad = (int64_t)st[6]; out->tail_exact = (int64_t)st[7];
    out->walk_cycles = (int64_t)st[LPC_STATS_CYC]; out->drain_cycles = (int64_t)st[LPC_STATS_CYC + 1];
    out->fan_exact = (int64_t)st[LPC_STATS_CYC + 2];
    out->behind_exact = (int64_t)st[LPC_STATS_CYC + 3];
    out->hit_exact = (int64_t)st[LPC_STATS_CYC + 4];
    out->heavy_piece = -1; out->heavy_piece_ticks = 0; out->piece_ticks = 0;
    for (int p = 0; p < LPC_STATS_PIECES; ++p) {
        const int64_t v = (int64_t)st[LPC_STATS_PIECE + p];
        out->piece_ticks += v;
        if (v > out->heavy_piece_ticks) { out->heavy_piece_ticks = v; out->heavy_piece = p; }
    }
    if (reset) {
        h->prof.isect_ms = h->prof.rest_ms = h->prof.kern_ms = 0.0; h->prof.launches = h->prof.pairs = 0;
        h->xchg_us = 0.0; h->xchg_calls = 0;
        if (h->prof.d_stats.p) HIPCHK(h, hipMemset(h->prof.d_stats.p, 0, LPC_STATS_WORDS * 8));
    }
    return 0;
}

// ---- light sources born on the device (light_source.py:98-188) ---------------
// The generator's state travels through d_mt (key[624] | pos), its doubles stay
// in d_rng; both kernels queue on the handle's stream.  mt_collect waits for them
// and reads the advanced state back.
static int mt_enqueue(lpc_handle *h, const char *who, const uint32_t *key, const int32_t *pos, int64_t n, bool fill)
{
    if (!key || !pos) return set_err(h, LPC_E_ARG, std::string(who) + ": key or pos is NULL");
    if (*pos < 0 || *pos > LPC_MT_N) return set_err(h, LPC_E_ARG, std::string(who) + ": pos outside 0..624");
    if (n < 0 || n > ((int64_t)1 << 60)) return set_err(h, LPC_E_ARG, std::string(who) + ": bad draw count");
    HIPCHK(h, hipSetDevice(h->device));
    RETIF(dalloc(h, h->d_mt, (LPC_MT_N + 1) * 4));
    if (fill) RETIF(dalloc(h, h->d_rng, (size_t)n * 8));
    uint32_t st[LPC_MT_N + 1];
    memcpy(st, key, LPC_MT_N * 4);
    st[LPC_MT_N] = (uint32_t)*pos;
    HIPCHK(h, hipStreamSynchronize(h->stream));      // d_mt may still be read by an earlier call's kernel
    HIPCHK(h, hipMemcpy(h->d_mt.p, st, sizeof(st), hipMemcpyHostToDevice));
    if (n > 0) {
        hipLaunchKernelGGL(k_mt19937, dim3(1), dim3(LPC_MT_THREADS), 0, h->stream, (uint32_t *)h->d_mt.p,
                           (int32_t *)h->d_mt.p + LPC_MT_N, n, fill ? (double *)h->d_rng.p : (double *)nullptr);
        HIPCHK(h, hipGetLastError());
    }
    return 0;
}

static int mt_collect(lpc_handle *h, uint32_t *key, int32_t *pos)
{
    uint32_t st[LPC_MT_N + 1];
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(st, h->d_mt.p, sizeof(st), hipMemcpyDeviceToHost));
    memcpy(key, st, LPC_MT_N * 4);
    *pos = (int32_t)st[LPC_MT_N];
    return 0;
}

int lpc_rng_mt19937(lpc_handle *h, uint32_t *key, int32_t *pos, int64_t n, double *host_out)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(mt_enqueue(h, "rng_mt19937", key, pos, n, host_out != nullptr));
    RETIF(mt_collect(h, key, pos));
    if (host_out && n > 0) HIPCHK(h, hipMemcpy(host_out, h->d_rng.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

// A device-resident source: (n,4) origin and direction rows and power[n] in plain
// device memory, the float64 sum of its powers, and an event the last kernel that
// wrote it recorded (a consumer on another stream waits on it).
struct lpc_rays {
    int device = 0;
    DBuf origin_rows, dir_rows, pow_vals;
    int64_t n = 0;
    double power_sum = 0.0;
    Event ready;
    float4 *origin() const { return (float4 *)origin_rows.p; }
    float4 *dir() const { return (float4 *)dir_rows.p; }
    float *pow() const { return (float *)pow_vals.p; }
};

static void rays_destroy(lpc_rays *r)
{
    if (r && r->ready) (void)hipEventSynchronize(r->ready);    // its last writer ends before the rows go
    delete r;
}

static int rays_create(lpc_handle *h, int64_t n, lpc_rays **out)
{
    std::unique_ptr<lpc_rays> r(new lpc_rays());
    r->device = h->device;
    r->n = n;
    const size_t rows = (size_t)std::max<int64_t>(n, 1);
    hipError_t e = r->origin_rows.alloc(rows * 16);
    if (e == hipSuccess) e = r->dir_rows.alloc(rows * 16);
    if (e == hipSuccess) e = r->pow_vals.alloc(rows * 4);
    if (e == hipSuccess) e = r->ready.create();
    if (e != hipSuccess)
        return set_err(h, LPC_E_NOMEM, std::string("device source of ") + std::to_string(n) + " rays: " +
                                           hipGetErrorString(e));
    *out = r.release();
    return 0;
}

static int emit_check(lpc_handle *h, const char *who, int64_t n, int64_t first, int64_t count, const float *center4,
                      const double *Rx9, const double *Rz9, lpc_rays **out)
{
    if (!center4 || !Rx9 || !Rz9 || !out) return set_err(h, LPC_E_ARG, std::string(who) + ": null argument");
    if (n < 1) return set_err(h, LPC_E_ARG, std::string(who) + ": n < 1");
    if (first < 0 || count < 0 || first > n || count > n - first)
        return set_err(h, LPC_E_ARG, std::string(who) + ": shard [first, first + count) outside [0, n]");
    return 0;
}

// hemisphere: the generator, the weights' sum, the shard's rays and their power
// sum, all queued on the stream; one wait at the end
static int emit_hemisphere(lpc_handle *h, lpc_rays *r, uint32_t *key, int32_t *pos, EmitArgs A)
{
    RETIF(mt_enqueue(h, "emit_hemisphere", key, pos, 2 * A.n, true));
    const int64_t nt = (A.n + LPC_EMIT_TILE - 1) / LPC_EMIT_TILE, nb = (A.count + 255) / 256;
    RETIF(dalloc(h, h->d_etile, (size_t)(2 + nt + nb) * 8));
    double *sums = (double *)h->d_etile.p, *wt = sums + 2, *pt = wt + nt;
    A.draws = (const double *)h->d_rng.p;
    A.wsum = sums;
    A.tile = pt;
    hipLaunchKernelGGL(k_emit_weights, dim3((unsigned)nt), dim3(256), 0, h->stream, A.draws, A.n, A.m, wt);
    hipLaunchKernelGGL(k_sum_tiles, dim3(1), dim3(256), 0, h->stream, (const double *)wt, nt, sums);
    if (nb > 0) hipLaunchKernelGGL(k_emit_hemisphere, dim3((unsigned)nb), dim3(256), 0, h->stream, A);
    hipLaunchKernelGGL(k_sum_tiles, dim3(1), dim3(256), 0, h->stream, (const double *)pt, nb, sums + 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(r->ready, h->stream));
    RETIF(mt_collect(h, key, pos));
    HIPCHK(h, hipMemcpy(&r->power_sum, sums + 1, 8, hipMemcpyDeviceToHost));
    return 0;
}

static int emit_collimated(lpc_handle *h, lpc_rays *r, uint32_t *key, int32_t *pos, EmitArgs A)
{
    RETIF(mt_enqueue(h, "emit_collimated", key, pos, 2 * A.n, true));
    A.draws = (const double *)h->d_rng.p;
    const int64_t nb = (A.count + 255) / 256;
    if (nb > 0) hipLaunchKernelGGL(k_emit_collimated, dim3((unsigned)nb), dim3(256), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(r->ready, h->stream));
    RETIF(mt_collect(h, key, pos));
    r->power_sum = (double)A.power * (double)A.count;
    return 0;
}

extern "C" {

int lpc_rays_emit_hemisphere(lpc_handle *h, uint32_t *key, int32_t *pos, int64_t n, int64_t first, int64_t count,
                             const float *center4, const double *Rx9, const double *Rz9, double power, double m,
                             lpc_rays **out)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(emit_check(h, "emit_hemisphere", n, first, count, center4, Rx9, Rz9, out));
    if (!(m >= 0.0)) return set_err(h, LPC_E_ARG, "emit_hemisphere: directivity exponent m < 0");
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    EmitArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.first = first; A.count = count;
    memcpy(A.Rx, Rx9, sizeof(A.Rx));
    memcpy(A.Rz, Rz9, sizeof(A.Rz));
    memcpy(A.center, center4, sizeof(A.center));
    A.power = (float)power;
    A.m = m;
    lpc_rays *r = nullptr;
    RETIF(rays_create(h, count, &r));
    A.origin = r->origin(); A.dirs = r->dir(); A.pow = r->pow();
    const int rc = emit_hemisphere(h, r, key, pos, A);
    if (rc) { rays_destroy(r); return rc; }
    *out = r;
    return 0;
}

int lpc_rays_emit_collimated(lpc_handle *h, uint32_t *key, int32_t *pos, int64_t n, int64_t first, int64_t count,
                             double diameter, const float *center4, const double *Rx9, const double *Rz9,
                             const float *dir_row3, double power, lpc_rays **out)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(emit_check(h, "emit_collimated", n, first, count, center4, Rx9, Rz9, out));
    if (!dir_row3) return set_err(h, LPC_E_ARG, "emit_collimated: null argument");
    *out = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    EmitArgs A;
    memset(&A, 0, sizeof(A));
    A.n = n; A.first = first; A.count = count;
    memcpy(A.Rx, Rx9, sizeof(A.Rx));
    memcpy(A.Rz, Rz9, sizeof(A.Rz));
    memcpy(A.center, center4, sizeof(A.center));
    memcpy(A.dir, dir_row3, sizeof(A.dir));
    // equal powers: ones * float32(power) / float32(sum of n ones)
    A.power = emit_power(1.0f, (float)power, (float)(double)n);
    A.diameter = diameter;
    lpc_rays *r = nullptr;
    RETIF(rays_create(h, count, &r));
    A.origin = r->origin(); A.dirs = r->dir(); A.pow = r->pow();
    const int rc = emit_collimated(h, r, key, pos, A);
    if (rc) { rays_destroy(r); return rc; }
    *out = r;
    return 0;
}

int lpc_rays_rotate(lpc_handle *h, lpc_rays *r, const double *R9, const double *pivot4)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (!r || !R9 || !pivot4) return set_err(h, LPC_E_ARG, "rays_rotate: null argument");
    if (r->device != h->device) return set_err(h, LPC_E_ARG, "rays_rotate: the source lives on another device");
    HIPCHK(h, hipSetDevice(h->device));
    if (r->n > 0) {
        RotateArgs A;
        A.n = r->n;
        memcpy(A.R, R9, sizeof(A.R));
        memcpy(A.piv, pivot4, sizeof(A.piv));
        A.origin = r->origin(); A.dirs = r->dir();
        HIPCHK(h, hipStreamWaitEvent(h->stream, r->ready, 0));
        hipLaunchKernelGGL(k_rays_rotate, dim3(grid1(r->n)), dim3(256), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(r->ready, h->stream));
    }
    return 0;
}

int lpc_rays_info(const lpc_rays *r, int64_t *n, double *power_sum)
{
    if (!r) return set_err(nullptr, LPC_E_ARG, "rays_info: null source");
    if (n) *n = r->n;
    if (power_sum) *power_sum = r->power_sum;
    return 0;
}

int lpc_rays_fetch(lpc_handle *h, const lpc_rays *r, float *origin4, float *dir4, float *pow)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    if (!r) return set_err(h, LPC_E_ARG, "rays_fetch: null source");
    HIPCHK(h, hipSetDevice(r->device));
    HIPCHK(h, hipEventSynchronize(r->ready));
    if (r->n > 0) {
        if (origin4) HIPCHK(h, hipMemcpy(origin4, r->origin(), (size_t)r->n * 16, hipMemcpyDeviceToHost));
        if (dir4) HIPCHK(h, hipMemcpy(dir4, r->dir(), (size_t)r->n * 16, hipMemcpyDeviceToHost));
        if (pow) HIPCHK(h, hipMemcpy(pow, r->pow(), (size_t)r->n * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(h, hipSetDevice(h->device));
    return 0;
}

int lpc_rays_free(lpc_rays *r)
{
    if (!r) return 0;
    (void)hipSetDevice(r->device);
    rays_destroy(r);
    return 0;
}

int lpc_trace_set_rays_dev(lpc_handle *h, lpc_rays *const *list, int32_t count, float max_ray_len, float ior_env)
{
    if (!h) return set_err(nullptr, LPC_E_ARG, "null handle");
    RETIF(settle(h));                   // a trace still running (lpc_trace_iterate / _run_async)
    RETIF(need_scene(h));
    if (count < 0 || (count > 0 && !list)) return set_err(h, LPC_E_ARG, "set_rays_dev: missing source list");
    int64_t n = 0;
    for (int32_t k = 0; k < count; ++k) {
        if (!list[k]) return set_err(h, LPC_E_ARG, "set_rays_dev: null source");
        if (list[k]->device != h->device)
            return set_err(h, LPC_E_ARG, "set_rays_dev: a source lives on another device");
        n += list[k]->n;
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    RETIF(pop_reserve(h, h->I, std::max<int64_t>(n, 1)));
    if (n > 0) {
        // the sources in list order, device to device; each after its producer's
        // last kernel (an event of the producing stream, no host wait)
        int64_t off = 0;
        for (int32_t k = 0; k < count; ++k) {
            const lpc_rays *r = list[k];
            if (r->n == 0) continue;
            HIPCHK(h, hipStreamWaitEvent(h->stream, r->ready, 0));
            unpack_rays(h->stream, r->n, (const float4 *)r->origin(), (const float4 *)r->dir(), h->I.f(0) + off,
                        (size_t)h->I.cap);
            HIPCHK(h, hipMemcpyAsync(h->I.f(6) + off, r->pow(), (size_t)r->n * 4, hipMemcpyDeviceToDevice, h->stream));
            off += r->n;
        }
        HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->I.pmid(), -2, (size_t)n, h->stream));
    }
    RayScan S;
    RETIF(ray_scan(h, h->I.in(), n, h->d_scan, &S));
    return emitted_rays(h, n, S, max_ray_len, ior_env);
}

}  // extern "C"
