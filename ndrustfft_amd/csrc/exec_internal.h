// exec_internal.h -- what exec.hip (device dispatch) shares with compose.hip (the weighted and filter calls, the batch-dim peel) and host.hip (the
// host-array call): one canonicalised problem, its dispatch, and the per-thread, per-device workspace.  Included by those three units only.
#pragma once
#include "engine.h"

namespace ndfft {

struct BatchDim { int64_t shape, sin, sout; };

struct Problem {
    const ndfft_plan *plan;
    int op;
    int64_t xlen, ylen;          // lane lengths
    int64_t xs, ys;              // axis strides
    std::vector<BatchDim> b;     // merged batch dims, slowest first
    int64_t nlanes;
    double scale;
    int keep_out = 0;            // column kernels: cache-allocating stores (the output is re-read right away, col_split)
    int stream_in = 0;           // column kernels: streaming loads (the input must not evict a cache-resident intermediate)
    int no_xcd_map = 0;          // column kernels: identity workgroup -> tile map (the stages of col_split: the map cost 7-20 us there)
    int makhoul_out = 0;         // column C2R kernels: outputs through the inverse of Makhoul's permutation (last pass of real_fourstep_inv, DCT-III)
};

inline size_t real_size(int dtype) { return dtype == NDFFT_F32 ? 4 : 8; }
inline bool op_in_cplx(int op) { return op == NDFFT_OP_C2C_FWD || op == NDFFT_OP_C2C_INV || op == NDFFT_OP_C2R; }
inline bool op_out_cplx(int op) { return op == NDFFT_OP_C2C_FWD || op == NDFFT_OP_C2C_INV || op == NDFFT_OP_R2C; }

// validation shared by the host and device entry points; fills Problem.  `nothing`: the call is valid and has nothing to do.
int prepare(const ndfft_plan *plan, int op, int ndim, const int64_t *shape_in, const int64_t *stride_in, const int64_t *shape_out,
            const int64_t *stride_out, int axis, int norm, double scale, Problem &P, bool &nothing);
// runs one problem on device arrays; more than kMaxBatchDims un-mergeable batch dims are peeled on the host (compose.hip)
int dispatch_peeled(Problem &P, const char *d_in, char *d_out, size_t ein, size_t eout, hipStream_t stream);

// ---- exec.hip, for compose.hip ----
// one problem of at most kMaxBatchDims batch dims on the first route that takes it
int dispatch(const Problem &P, const void *d_in, void *d_out, hipStream_t stream);
// a route that ran another dispatch() inside: its path is "<prefix><inner path>"
int prefixed(const char *prefix, int rc);
// scratch array `which` (DeviceWs::scratch) of this thread on stream s, at least `bytes` long
int get_scratch(int which, hipStream_t s, size_t bytes, void **out);
// load policy of a dense row kernel that reads `bytes` at `in` and writes as many at `out` (Pow2Args::stream_in), and the model's bookkeeping for the next call
// keep64: the pow2 row kernel's kept share of a streamed input (Pow2Args::keep64; MallModel below) -- callers whose kernel streams everything pass none
int c2c_row_load_policy(const void *in, const void *out, size_t bytes, int *keep64 = nullptr, bool grant = true);
void reset_last_policy();         // every entry point, first thing: ndfft_last_input_policy answers for this call

// The lane layout of one call: lane L = (o, i) with i the fastest batch dimension, element j of it at o * outer + i * lane + j * elem.
// (dense compares the pitches with the lane lengths xlen / ylen: for C2C both are n)
struct Layout {
    bool rows;                       // unit element stride on both sides and one batch dimension at most: lanes at a uniform pitch
    bool dense;                      // ... and that pitch is the lane length on both sides
    bool cols;                       // the fastest batch dimension has unit stride on both sides: adjacent lanes are contiguous
    int64_t pitch_in, pitch_out;     // stride of the slowest batch dimension (the lane pitch of rows), the lane length without one
    int64_t inner;                   // extent of i (1 without a batch dimension)
    int64_t lane_in, lane_out;       // stride of i (0 without a batch dimension)
    int64_t outer_in, outer_out;     // stride of o: the slower of two batch dimensions (0 with fewer)
    explicit Layout(const Problem &P) {
        const size_t nb = P.b.size();
        rows = P.xs == 1 && P.ys == 1 && nb <= 1;
        pitch_in = nb ? P.b[0].sin : P.xlen; pitch_out = nb ? P.b[0].sout : P.ylen;
        dense = rows && pitch_in == P.xlen && pitch_out == P.ylen;
        cols = nb && P.b.back().sin == 1 && P.b.back().sout == 1;
        inner = nb ? P.b.back().shape : 1;
        lane_in = nb ? P.b.back().sin : 0; lane_out = nb ? P.b.back().sout : 0;
        outer_in = nb == 2 ? P.b[0].sin : 0; outer_out = nb == 2 ? P.b[0].sout : 0;
    }
};

// A route (of dispatch() in exec.hip, of ndfft_exec in host.hip) returns NDFFT_OK, a real error (returned to the caller), or kDeclined:
// "not mine, the next route runs".  kDeclined is no ndfft status and never leaves the function that walks the routes.
constexpr int kDeclined = -1;

// ---------------------------------------------------------------------------------------------
// Workspace of one host thread ON ONE DEVICE: scratch arrays of the multi-pass routes (keyed by stream; they
// grow, never shrink), the staging buffers and pinned bounce buffers of ndfft_exec, and the streams / events of
// its chunk pipeline.  A thread that alternates ndfft_set_device gets one of these per device (nothing allocated
// on device 0 is ever handed to a kernel on device 1), and everything is released when the thread exits.
// ---------------------------------------------------------------------------------------------
struct Scratch { void *p = nullptr; size_t cap = 0; };
struct Staging {
    void *p = nullptr; size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return NDFFT_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        NDFFT_HIP(hipMalloc(&p, bytes));
        cap = bytes;
        return NDFFT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
struct PinnedBuf {
    void *p = nullptr; size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return NDFFT_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        NDFFT_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
        cap = bytes;
        return NDFFT_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};
struct Pipe {
    hipStream_t h2d = nullptr, cmp = nullptr, d2h = nullptr;
    std::vector<hipEvent_t> up, done, down;
    bool ok = false;
    void sync_all() { if (ok) { (void)hipStreamSynchronize(h2d); (void)hipStreamSynchronize(cmp); (void)hipStreamSynchronize(d2h); } }
    void release() {
        if (!ok) return;
        sync_all();
        for (auto *v : {&up, &done, &down}) { for (hipEvent_t e : *v) (void)hipEventDestroy(e); v->clear(); }
        (void)hipStreamDestroy(h2d); (void)hipStreamDestroy(cmp); (void)hipStreamDestroy(d2h);
        h2d = cmp = d2h = nullptr; ok = false;
    }
};
// What this thread's own calls imply about the 256 MiB Infinity Cache of the current device -- used for ONE decision, the load
// policy of the row / column-tile kernels that have a streaming-load form (BASELINE configs[1], [3], [4]): plain loads are up to 15 %
// faster when the input is resident in the Infinity Cache (4096 x 4096 c128: 0.86 vs 0.74 of the roofline), streaming (nt) loads 6 %
// faster when it comes from HBM (0.74 vs 0.70).  Round 2 bet on "resident" for every input <= 384 MiB; a chain of nd* calls loses that bet
// at every link (the output of a pass was written with nt stores, which bypass the cache).  The model is an LRU stack distance per buffer
// this thread has transformed:
//   * a buffer this thread WROTE as an output of more than 64 MiB is cold (nt stores) -> streaming loads when it becomes an input;
//   * a buffer it READ before (with either policy), or wrote as a small output, is worth plain loads iff the bytes this thread has moved
//     through the cache since (all inputs, small outputs) plus its own size fit ~256 MiB: a re-read input then is, or becomes, resident;
//     six rotating 256 MiB inputs never are (streaming loads for all of them, each with a kept share: below);
//   * a buffer the model has never seen keeps round 2's size rule (plain loads up to 384 MiB) -- its producer is unknown.
// A stale entry (the allocator reused the addresses for something a foreign kernel produced) costs one call: after that the buffer is "read".
// ndfft_set_input_hint overrides the model per host thread.  Speed only: either policy gives the same results.
//
// The kept share.  LRU is the wrong policy for a CYCLE larger than the cache: it answers a rotation of inputs with "streaming loads for all of them", nothing
// allocates and the cache sits idle.  Pinning a fixed subset gives a hit rate of cache / footprint instead of 0, and software can pin, because streaming (nt)
// accesses do not allocate and plain loads do.  So a dense row-kernel input that the model STREAMS and has seen being READ before -- its reuse distance D = the
// bytes moved through the cache since its last read plus its own size, the quantity decide() forms, exceeds the cache; or it is larger than the cache, the size-rule
// path -- gets keep64 = floor(64 kKeepBudget / D), at most 63: that many of every 64 blocks of 64 KiB (device_common.h: keep_block, a fixed, evenly spread,
// nested choice) are loaded with the default policy.  Every member of a rotation then keeps budget / D of itself, kKeepBudget in all, and finds it resident the next
// time round.  The share is 0 for a buffer last written past the cache (OUT_COLD), an unknown buffer, NDFFT_INPUT_COLD (the caller says the data is not there) and a
// policy forced by NDFFT_STREAM_LOADS.  The clock still counts every input byte read, kept or not: conservative.  Worst case: kept lanes that miss (a foreign
// producer rewrote the buffers; the first cycle after the grant) cost what plain loads cost on a cold input, 6 % of their share.
// c128 rows only: c64 rows of 8192 points (BASELINE configs[2], second transform: three rotating 268 MB inputs) ran 95.7 / 96.7 -> 99.2 / 97.6 us with the model's share of
// 15, so f32 plans are granted none.  ndfft_set_keep_budget sets the budget per host thread (0: the feature is off), ndfft_force_input_keep forces the share of every
// streamed dense input, f32 included (tests, sweeps; the developer build reads NDFFT_KEEP_BUDGET_MB / NDFFT_KEEP64).
struct MallModel {
    enum State { READ = 0, OUT_SMALL = 1, OUT_COLD = 2 };
    struct Entry { uintptr_t lo, hi; uint64_t stamp; int state; };
    std::vector<Entry> e;
    uint64_t clock = 0;                          // bytes this thread has moved through the cache's address stream (inputs read, small outputs)
    static constexpr uint64_t kCap = (uint64_t)256 << 20, kSmallOut = (uint64_t)64 << 20;
    // what the kept shares of the members of a rotation add up to.  Swept on the six rotating 4096 x 4096 c128 pairs (profiles/r16/budget_sweep.txt):
    // 0 / 96 / 144 / 192 / 216 / 240 / 288 / 384 MiB kept -> 90.5 / 89.2 / 88.8 / 87.6 / 87.7 / 88.7 / 89.7 / 89.8 us; 216 MiB is still at the best time and the
    // next step is not, so the budget stays one step below it
    static constexpr uint64_t kKeepBudget = (uint64_t)192 << 20;
    // kept share (Pow2Args::keep64) of input `in`, which decide() did not answer with plain loads; before note_read
    int share(const void *in, size_t bytes, uint64_t budget) {
        const Entry *x = find(in, bytes);
        if (!x || x->state != READ || bytes == 0) return 0;
        const uint64_t d = clock - x->stamp + bytes;
        return (int)std::min<uint64_t>(63, 64 * budget / d);
    }
    Entry *find(const void *p, size_t bytes) {
        const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
        for (auto &x : e) if (lo < x.hi && x.lo < hi) return &x;
        return nullptr;
    }
    // 1: streaming loads, 0: plain loads, -1: unknown buffer (the launcher decides by size)
    int decide(const void *in, size_t bytes) {
        const Entry *x = find(in, bytes);
        if (!x) return -1;
        if (x->state == OUT_COLD) return 1;
        // a buffer larger than the cache (BASELINE configs[2]'s 4097 x 8192 c64 is 64 KiB over): only an IMMEDIATE re-read still finds most of it
        // there (the size rule decides, as for an unknown buffer); anything else this thread has read since has pushed it out -- round 5: the
        // rotating-pairs table ran this shape with plain loads (policy 0), 95.9 us against 92 us with streaming loads
        if (bytes > kCap) return clock == x->stamp ? -1 : 1;
        return clock - x->stamp + bytes <= kCap ? 0 : 1;
    }
    void put(const void *p, size_t bytes, int state, bool through_cache) {
        const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
        for (size_t i = 0; i < e.size();) { if (lo < e[i].hi && e[i].lo < hi) e.erase(e.begin() + i); else ++i; }
        if (through_cache) clock += bytes;
        if (e.size() >= 32) e.erase(e.begin());  // oldest first
        e.push_back({lo, hi, clock, state});
    }
    void note_read(const void *p, size_t bytes) { put(p, bytes, READ, true); }
    void note_write(const void *p, size_t bytes) { if (bytes <= kSmallOut) put(p, bytes, OUT_SMALL, true); else put(p, bytes, OUT_COLD, false); }
};
struct DeviceWs {
    MallModel mall;
    std::map<hipStream_t, Scratch> scratch[9];   // 0..7: the multi-pass routes; 8: the image a weight pass writes ahead of the transform (compose.hip: weighted, filter_composed)
    Staging stage_in, stage_out;
    PinnedBuf bounce_in[3], bounce_out[3];
    Pipe pipe;
    void release() {   // the owning device must be current
        pipe.release();
        for (auto &m : scratch) { for (auto &kv : m) if (kv.second.p) (void)hipFree(kv.second.p); m.clear(); }
        stage_in.release(); stage_out.release();
        for (auto &b : bounce_in) b.release();
        for (auto &b : bounce_out) b.release();
    }
};
int current_ws(DeviceWs **out);   // this thread's workspace on the current device (created on first use; released by ndfft_release_workspace / thread exit)

}  // namespace ndfft
