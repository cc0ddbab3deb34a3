// exec.hip -- ndfft_exec_device and what every nd* call shares: the body of one call on device arrays.
// Replaces the reference's lane iterator (create_transform! src/lib.rs:100-167 and its _par twin
// 169-238): validation that mirrors the reference's panics, stride canonicalisation (the three
// iterator strategies collapse into "every lane along `axis`, arbitrary signed strides") and kernel choice.  Host arrays are staged
// through HBM by host.hip (ndfft_exec), which comes back here for prepare() and dispatch() (exec_internal.h); the calls composed of dispatch() and a pass
// around it -- the batch-dim peel, Normalization::Weights, the filters -- are compose.hip's.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>

#include "exec_internal.h"
#include "pow2_real.h"
#include "../../include/ndfft_mi355x_ext.h"

namespace ndfft {

static int kind_of_op(int op) {
    if (op == NDFFT_OP_C2C_FWD || op == NDFFT_OP_C2C_INV) return NDFFT_KIND_C2C;
    if (op == NDFFT_OP_R2C || op == NDFFT_OP_C2R) return NDFFT_KIND_R2C;
    return NDFFT_KIND_DCT;
}

// kernel op (generic_kernel.h: G_*) and plan slot of an nd* op on a lane of n points
static int gen_op_of(int op, int n, int *slot) {
    *slot = CFG_MAIN;
    switch (op) {
        case NDFFT_OP_C2C_FWD: return G_C2C_FWD;
        case NDFFT_OP_C2C_INV: return G_C2C_INV;
        case NDFFT_OP_R2C: return n % 2 ? G_R2C_ODD : G_R2C_EVEN;
        case NDFFT_OP_C2R: return n % 2 ? G_C2R_ODD : G_C2R_EVEN;
        case NDFFT_OP_DCT1: if (n == 1) return G_DCT2_ODD; *slot = CFG_DCT1; return G_DCT1;
        case NDFFT_OP_DCT2: return n % 2 ? G_DCT2_ODD : G_DCT2_EVEN;
        case NDFFT_OP_DCT3: return n % 2 ? G_DCT3_ODD : G_DCT3_EVEN;
        default: *slot = CFG_DCT4; return n % 2 ? G_DCT4_ODD : G_DCT4_EVEN;
    }
}

// validation shared by the host and device entry points; fills Problem. Returns 1 for "nothing to do".
int prepare(const ndfft_plan *plan, int op, int ndim, const int64_t *shape_in, const int64_t *stride_in,
            const int64_t *shape_out, const int64_t *stride_out, int axis, int norm, double scale,
            Problem &P, bool &nothing) {
    nothing = false;
    if (!plan) return fail(NDFFT_ERR_INVALID_ARG, "plan is null");
    if (op < NDFFT_OP_C2C_FWD || op > NDFFT_OP_DCT4) return fail(NDFFT_ERR_INVALID_ARG, "bad op");
    if (kind_of_op(op) != plan->kind) return fail(NDFFT_ERR_INVALID_ARG, "op does not belong to this plan's handler kind");
    if (norm < NDFFT_NORM_NONE || norm > NDFFT_NORM_SCALE) return fail(NDFFT_ERR_INVALID_ARG, "bad norm");
    if (ndim < 0 || ndim > NDFFT_MAX_DIMS) return fail(NDFFT_ERR_INVALID_ARG, "ndim out of range");
    if (ndim && (!shape_in || !stride_in || !shape_out || !stride_out)) return fail(NDFFT_ERR_INVALID_ARG, "null shape/stride");
    // lib.rs:116  let n = output.shape()[axis];
    if (axis < 0 || axis >= ndim) {
        char m[96];
        snprintf(m, sizeof m, "index out of bounds: the len is %d but the index is %d", ndim, axis);
        return fail(NDFFT_ERR_AXIS, m);
    }
    // Zip::from(input.rows()).and(output.rows_mut()) needs equal producer shapes (lib.rs:120-121)
    std::vector<BatchDim> raw;
    P.nlanes = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape_in[d] < 0 || shape_out[d] < 0) return fail(NDFFT_ERR_INVALID_ARG, "negative extent");
        if (d == axis) continue;
        if (shape_in[d] != shape_out[d]) {
            char m[128];
            snprintf(m, sizeof m, "ndarray: Zip dimension mismatch on axis %d (%lld vs %lld)", d, (long long)shape_in[d],
                     (long long)shape_out[d]);
            return fail(NDFFT_ERR_SHAPE_MISMATCH, m);
        }
        P.nlanes *= shape_in[d];
        if (shape_in[d] != 1) raw.push_back({shape_in[d], stride_in[d], stride_out[d]});
    }
    P.plan = plan; P.op = op;
    P.xlen = shape_in[axis]; P.ylen = shape_out[axis];
    P.xs = stride_in[axis]; P.ys = stride_out[axis];
    if (P.nlanes == 0) { nothing = true; return NDFFT_OK; }   // the closure never runs: no size panic either
    // the lane method's asserts: data.len() first, then out.len() (lib.rs:314-315, 498-499, 507-508, 689-690)
    const int64_t want_in = (int64_t)ndfft_plan_lane_len_in(plan, op), want_out = (int64_t)ndfft_plan_lane_len_out(plan, op);
    const char *what = plan->kind == NDFFT_KIND_DCT ? "dct" : "fft";
    if (P.xlen != want_in || P.ylen != want_out) {
        char m[128];
        const bool in_bad = P.xlen != want_in;
        snprintf(m, sizeof m, "Size mismatch in %s, got %lld expected %lld", what,
                 (long long)(in_bad ? P.xlen : P.ylen), (long long)(in_bad ? want_in : want_out));
        return fail(NDFFT_ERR_SIZE_MISMATCH, m);
    }
    if (plan->n == 0) { nothing = true; return NDFFT_OK; }
    // merge adjacent batch dims that are contiguous in both views
    for (const BatchDim &d : raw) {
        if (!P.b.empty()) {
            BatchDim &p = P.b.back();
            if (p.sin == d.shape * d.sin && p.sout == d.shape * d.sout) {
                p.shape *= d.shape; p.sin = d.sin; p.sout = d.sout;
                continue;
            }
        }
        P.b.push_back(d);
    }
    // normalisation scalar at the reference's application point
    const double n = (double)plan->n;
    switch (op) {
        case NDFFT_OP_C2C_FWD: case NDFFT_OP_R2C: P.scale = 1.0; break;                         // ignored: lib.rs:313-318, 497-503
        case NDFFT_OP_C2C_INV: case NDFFT_OP_C2R:                                               // lib.rs:333-338, 525-531
            P.scale = norm == NDFFT_NORM_NONE ? 1.0 : norm == NDFFT_NORM_DEFAULT ? 1.0 / n : scale; break;
        default:                                                                                 // lib.rs:736-741
            P.scale = norm == NDFFT_NORM_NONE ? 1.0 : norm == NDFFT_NORM_DEFAULT ? 2.0 : scale; break;
    }
    return NDFFT_OK;
}

int validate_call(const ndfft_plan *plan, int op, int ndim, const int64_t *shape_in, const int64_t *stride_in, const int64_t *shape_out,
                  const int64_t *stride_out, int axis, int norm, double scale, bool *nothing) {
    Problem P;
    return prepare(plan, op, ndim, shape_in, stride_in, shape_out, stride_out, axis, norm, scale, P, *nothing);
}

// ---------------------------------------------------------------------------------------------
// dispatch of one canonicalised problem with <= kMaxBatchDims batch dims
// ---------------------------------------------------------------------------------------------
template <typename T>
static int dispatch_generic(const Problem &P, const void *d_in, void *d_out, const DevTables &dt, hipStream_t stream) {
    const ndfft_plan *plan = P.plan;
    const int n = (int)plan->n;
    GenArgs<T> a;
    memset(&a, 0, sizeof a);
    int slot;
    const int gop = gen_op_of(P.op, n, &slot);
    const FftConfig &c = plan->cfg[slot];
    const DevConfig &d = dt.cfg[slot];
    a.in = d_in; a.out = d_out;
    a.nlanes = P.nlanes;
    a.op = gop; a.n = n;
    a.n_in = (int)P.xlen; a.n_out = (int)P.ylen;
    a.in_cplx = op_in_cplx(P.op); a.out_cplx = op_out_cplx(P.op);
    a.F = c.F;
    a.npass = (int)c.radix.size();
    for (int i = 0; i < a.npass; ++i) a.radix[i] = c.radix[i];
    a.scale = (T)P.scale;
    a.tw = (const cpx<T> *)d.tw; a.aux1 = (const cpx<T> *)d.aux1; a.aux2 = (const cpx<T> *)d.aux2;
    a.blue = c.blue; a.M = c.M; a.npassM = (int)c.radixM.size();
    for (int i = 0; i < a.npassM; ++i) a.radixM[i] = c.radixM[i];
    a.twM = (const cpx<T> *)d.twM; a.chirp = (const cpx<T> *)d.chirp; a.bhat = (const cpx<T> *)d.bhat;

    a.gin.axis_stride = P.xs; a.gout.axis_stride = P.ys;
    a.gin.nb = a.gout.nb = (int)P.b.size();
    for (size_t i = 0; i < P.b.size(); ++i) {
        a.gin.bshape[i] = a.gout.bshape[i] = P.b[i].shape;
        a.gin.bstride[i] = P.b[i].sin; a.gout.bstride[i] = P.b[i].sout;
    }
    // thread -> (lane, element) map for global IO: along the lane if it is unit-stride, else across
    // adjacent lanes if the fastest batch dim is unit-stride (the fused LDS transpose), else row.
    const bool last_in1 = !P.b.empty() && P.b.back().sin == 1, last_out1 = !P.b.empty() && P.b.back().sout == 1;
    a.load_mode = (P.xs == 1 || P.xlen == 1 || !last_in1) ? IO_ROW : IO_COL;
    a.store_mode = (P.ys == 1 || P.ylen == 1 || !last_out1) ? IO_ROW : IO_COL;

    // LDS pitch (complex elements): the padded FFT buffer (or Bluestein M) and the raw input lane must fit
    const int in_c = a.in_cplx ? a.n_in : (a.n_in + 1) / 2;
    const int len = std::max(c.blue ? c.M : c.F, 1);
    const int pitch = std::max(generic_z_len(len), in_c) | 1;   // odd: lanes land in different banks for the IO_COL transposes
    const size_t csize = 2 * sizeof(T);
    const size_t lds_cap = 160 * 1024;
    if (generic_lds_bytes(1, pitch, csize, 2) > lds_cap) {
        char m[160];
        snprintf(m, sizeof m, "lane of %d elements needs %zu B of LDS (> %zu): multi-pass path not built yet", n,
                 generic_lds_bytes(1, pitch, csize), lds_cap);
        return fail(NDFFT_ERR_UNSUPPORTED, m);
    }
    const bool col = a.load_mode == IO_COL || a.store_mode == IO_COL;
    // threads per lane in the FFT phases: one butterfly each in the pass with the most butterflies
    int nb_max = 1;
    {
        const std::vector<int> &rr = c.blue ? c.radixM : c.radix;
        for (int r : rr) nb_max = std::max(nb_max, len / r);
    }
    const bool elementwise = gop == G_C2C_FWD || gop == G_C2C_INV || gop == G_R2C_EVEN || gop == G_R2C_ODD;
    // (the in-place and the prime-radix kernels are compiled for <= 512 threads: 256-VGPR budget)
    const bool want_inplace = elementwise && nb_max <= 512;
    const int maxthr = (want_inplace || generic_needs_big(a.radix, a.npass, a.radixM, a.blue ? a.npassM : 0)) ? 512 : 1024;
    int fft_tpl = 1; while (fft_tpl < nb_max && fft_tpl < maxthr) fft_tpl <<= 1;
    // in place (one LDS buffer per lane) when the op is elementwise at both ends and a thread never owns more
    // than one butterfly of a pass: needs fft_tpl >= nb_max and one thread group per lane
    const bool inplace = want_inplace && fft_tpl >= nb_max;
    const int nbuf = inplace ? 1 : 2;
    // lanes per block: fill ~64 KiB of LDS (2+ blocks/CU), but never more lanes than exist
    const size_t per_lane = (size_t)nbuf * (size_t)pitch * csize;
    int lpb = (int)std::min<size_t>((64 * 1024) / per_lane, kMaxLpb);
    if (col) {
        // want >= 128 B contiguous across lanes per row of the tile; take more LDS if that is what it costs
        const int want = (int)std::min<size_t>(kMaxLpb, std::max<size_t>(128 / sizeof(T) / (a.in_cplx ? 2 : 1), 16));
        const int fit = (int)std::min<size_t>((lds_cap - 2048) / per_lane, kMaxLpb);
        lpb = std::max(lpb, std::min(want, fit));
    }
    lpb = std::max(1, lpb);
    if (inplace) lpb = std::max(1, std::min(lpb, maxthr / fft_tpl));   // one thread group per lane
    if ((int64_t)lpb > P.nlanes) lpb = (int)P.nlanes;
    // keep every CU busy: prefer >= 1024 blocks when lanes allow
    while (lpb > 1 && !col && (P.nlanes + lpb - 1) / lpb < 1024) lpb = (lpb + 1) / 2;
    int lpb_log = 0;
    if (col) {   // the across-lanes thread map needs a power of two
        while ((2 << lpb_log) <= lpb) ++lpb_log;
        lpb = 1 << lpb_log;
    }
    a.lpb = lpb; a.pitch = pitch; a.lpb_log = lpb_log; a.inplace = inplace;
    const size_t lds = generic_lds_bytes(lpb, pitch, csize, nbuf);
    int threads = 64; while (threads < lpb * fft_tpl && threads < maxthr) threads <<= 1;
    if (col) while (threads < 4 * lpb && threads < maxthr) threads <<= 1;
    if (inplace && threads < lpb * fft_tpl) return fail(NDFFT_ERR_INVALID_ARG, "internal: in-place thread map");
    fft_tpl = std::min(fft_tpl, threads);
    int io_tpl = 1; while (io_tpl < std::max(a.n_in, a.n_out) && io_tpl < threads) io_tpl <<= 1;
    a.fft_tpl_log = 0; while ((1 << a.fft_tpl_log) < fft_tpl) ++a.fft_tpl_log;
    a.io_tpl_log = 0; while ((1 << a.io_tpl_log) < io_tpl) ++a.io_tpl_log;
    set_last_path(col ? "generic_col" : (P.xs == 1 || P.xlen == 1) && (P.ys == 1 || P.ylen == 1) ? "generic_row" : "generic_strided");
    return launch_generic<T>(a, threads, lds, stream);
}

// ---------------------------------------------------------------------------------------------
// The workspaces of one host thread (exec_internal.h: DeviceWs), one per device it has used, released in one place
// ---------------------------------------------------------------------------------------------
struct ThreadWs {
    std::map<int, DeviceWs> dev;
    void release_all() {
        if (dev.empty()) return;
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); dev.clear(); return; }   // runtime already gone (process teardown)
        for (auto &kv : dev) { if (hipSetDevice(kv.first) == hipSuccess) { (void)hipDeviceSynchronize(); kv.second.release(); } }
        (void)hipSetDevice(cur);
        dev.clear();
    }
    ~ThreadWs() { release_all(); }   // a worker thread that exits gives its device memory and streams back
};
static thread_local ThreadWs g_tws;
int current_ws(DeviceWs **out) {
    int dev = 0;
    NDFFT_HIP(hipGetDevice(&dev));
    *out = &g_tws.dev[dev];
    return NDFFT_OK;
}
static thread_local int g_input_hint = NDFFT_INPUT_AUTO;
static thread_local int g_last_policy = -1;       // load policy the last call on this thread asked the model for (diagnostic)
static thread_local int g_last_keep = 0;          // ... and the kept share (Pow2Args::keep64) it was given (diagnostic)
static thread_local int g_keep_budget_mb = -1;    // ndfft_set_keep_budget: MiB, -1 = MallModel::kKeepBudget
static thread_local int g_keep_force = -1;        // ndfft_force_input_keep: 0 .. 64, -1 = the model's share
void reset_last_policy() { g_last_policy = -1; g_last_keep = 0; }
static bool F_nt_ok(int F) { return F >= 64; }   // (short lanes: the staging loads are not 16-byte vectors on every path)
// load policy for the dense C2C row kernels on input `in` (Pow2Args::stream_in), and the bookkeeping for the next call (the model: exec_internal.h, MallModel)
// keep64 (the pow2 row kernel only): where the model grants the input a kept share (MallModel), that share; the other callers stream everything they stream
// (grant = false: the caller's kernel takes a forced share only -- c64 rows, where the model's share measured slower: DESIGN.md section 3.1)
static int row_load_policy(const void *in, size_t bytes, const void *out, size_t out_bytes, int *keep64 = nullptr, bool grant = true);
int c2c_row_load_policy(const void *in, const void *out, size_t bytes, int *keep64, bool grant) { return row_load_policy(in, bytes, out, bytes, keep64, grant); }
static int row_load_policy(const void *in, size_t bytes, const void *out, size_t out_bytes, int *keep64, bool grant) {
    const int force = sw().stream_loads;            // NDFFT_STREAM_LOADS: 0 / 1 forces a policy
    DeviceWs *ws;
    if (current_ws(&ws)) return -1;
    const bool model = force < 0 && g_input_hint == NDFFT_INPUT_AUTO;
    int pol = force >= 0 ? (force != 0) : g_input_hint == NDFFT_INPUT_CACHED ? 0 : g_input_hint == NDFFT_INPUT_COLD ? 1 : ws->mall.decide(in, bytes);
    const bool nt = pol >= 0 ? pol != 0 : stream_loads_for(bytes);
    g_last_policy = nt ? 1 : 0;
    if (keep64) {
        // the model's own "streaming", or its size-rule path for a buffer it knows (there the share is reported whatever the size rule says: with plain loads
        // every lane allocates anyway); NDFFT_KEEP64 forces the share of whatever streams
        // (per host thread, like the hint: ndfft_set_keep_budget / ndfft_force_input_keep; the developer build reads NDFFT_KEEP_BUDGET_MB / NDFFT_KEEP64 for sweeps)
        const int kb = g_keep_budget_mb >= 0 ? g_keep_budget_mb : (int)NDFFT_DEV_INT("NDFFT_KEEP_BUDGET_MB", -1);
        const int kf = g_keep_force >= 0 ? g_keep_force : (int)std::min<long>(64, NDFFT_DEV_INT("NDFFT_KEEP64", -1));
        const uint64_t budget = kb >= 0 ? (uint64_t)kb << 20 : MallModel::kKeepBudget;
        int k = grant && model && pol != 0 && budget ? ws->mall.share(in, bytes, budget) : 0;
        if (kf >= 0 && nt) k = kf;
        *keep64 = g_last_keep = k;
    }
    ws->mall.note_read(in, bytes);
    // nt stores: a large output bypasses the cache (fft -> ifft on 4096 x 4096 c128: the second pass is 3-5 % faster with streaming loads); a small
    // one is still found there (1024 x 4096, 64 MiB: plain loads 2-3 % faster) -- tools/probes/chain_hint.py, profiles/r05/r05d_chain_hint.txt
    ws->mall.note_write(out, out_bytes);
    return nt ? 1 : 0;
}
int get_scratch(int which, hipStream_t s, size_t bytes, void **out) {
    DeviceWs *ws;
    int rc = current_ws(&ws);
    if (rc) return rc;
    Scratch &sc = ws->scratch[which][s];
    if (bytes > sc.cap) {
        if (sc.p) { NDFFT_HIP(hipStreamSynchronize(s)); NDFFT_HIP(hipFree(sc.p)); sc.p = nullptr; sc.cap = 0; }
        NDFFT_HIP(hipMalloc(&sc.p, bytes));
        sc.cap = bytes;
    }
    *out = sc.p;
    return NDFFT_OK;
}

// (the result of a route: exec_internal.h, kDeclined)
// A hiprtc launcher's NDFFT_ERR_UNSUPPORTED (no hiprtc, a failed compile or module load, NDFFT_JIT=cached with nothing cached) declines its route.
static int jit_rc(int rc) { return rc == NDFFT_ERR_UNSUPPORTED ? kDeclined : rc; }
// a route's result: its path is recorded unless it declined
static int took(int rc, const char *path) {
    if (rc != kDeclined) set_last_path(path);
    return rc;
}

static int transpose_batched(const void *in, void *out, int64_t batch, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out,
                             int64_t bs_in, int64_t bs_out, int esz, hipStream_t s) {
    for (int64_t b0 = 0; b0 < batch; b0 += 32768) {   // grid.z limit
        const int64_t nb = std::min<int64_t>(32768, batch - b0);
        int rc = launch_transpose((const char *)in + b0 * bs_in * esz, (char *)out + b0 * bs_out * esz, nb, rows, cols, ld_in, ld_out,
                                  bs_in, bs_out, esz, s);
        if (rc) return rc;
    }
    return NDFFT_OK;
}


// Route switches (switches.h; parsed once, never read from the environment on the call path).  Each closes one route so that the kernel
// behind it runs: the parity tests reach every fallback kernel that way.
static bool narrow_dct_enabled() { return sw().narrow_dct; }               // NDFFT_NARROW_DCT=1: long strided DCT lanes on the narrow tiles again
static bool wave_enabled() { return sw().wave; }                           // NDFFT_WAVE=0: short dense C2C lanes on the older kernels
static bool fourstep2_enabled() { return sw().fourstep2; }                 // NDFFT_FOURSTEP2=0: long power-of-two lanes on the three-pass form
// NDFFT_REAL_FOURSTEP=0 keeps long real-data lanes on the packed complex four-step with separate PRE / POST passes
// (2 = for every eligible op, also where the plan's table says the packed route is faster: parity tests)
static int real_fourstep_enabled() { return sw().real_fourstep; }
// largest handler length the thread-per-lane real-op register kernels take (raw lane + Z + outputs in registers)
static int regreal_max_n(int f64) {
    return f64 ? (int)NDFFT_DEV_INT("NDFFT_REGREAL_MAX_F64", 48)           // f64 n = 48: 0.66 vs 0.30
               : (int)NDFFT_DEV_INT("NDFFT_REGREAL_MAX_F32", 72);          // f32 n = 64: 0.66 vs 0.50; n = 96 / 100: 0.39 / 0.37 vs 0.41 / 0.49
}
static bool tiny_enabled() { return sw().tiny; }                           // NDFFT_TINY=0: very short lanes on the LDS kernel
static bool plain_enabled() { return sw().plain; }                         // NDFFT_PLAIN=0: odd-n real ops with a smooth inner FFT on the LDS kernel
static bool blue_enabled() { return sw().blue; }                           // NDFFT_BLUE=0: Bluestein lengths on the LDS kernel
static bool colsplit_enabled() { return sw().colsplit; }                   // NDFFT_COLSPLIT=0: long strided lanes on the narrow-tile / transpose routes

template <typename T> static int dtype_of() { return sizeof(T) == 8 ? NDFFT_F64 : NDFFT_F32; }

// How one four-step pass (engine.h: FsPass) of length F runs, given the C2C or R2C sub-plan of that length: on the kernel compiled ahead of time for F, on one
// specialised with hiprtc from the sub-plan's recipe, or not at all -- and with which of the sub-plan's per-pass twiddle tables.
enum FsHow { FS_NONE = 0, FS_AOT, FS_RTC };
struct FsPlan {
    FsPass pass = FS_CPX_1; int F = 0; const ndfft_plan *sub = nullptr;
    FsHow how = FS_NONE;
    const JitCfg *recipe = nullptr;            // FS_RTC
    void *DevConfig::*twp = nullptr;           // the twiddle table of that form ...
    bool wide = false;                         // ... unless the pass runs the wide (E = 16) recipe on twp_col_w (kernels_fourstep.hip)
    explicit operator bool() const { return how != FS_NONE; }
};
static bool jit_col_ok(int dtype, const JitCfg &cfg) { return jit_col_lanes(dtype, cfg, false) > 0; }
static FsPlan fs_plan(FsPass pass, int F, const ndfft_plan *sub, int dtype) {
    const FftConfig &c = sub->cfg[CFG_MAIN];
    // What follows from the pass.  `rows`: an R2C sub-plan, the pass runs its rows' recipe and tables (a C2C sub-plan keeps separate ones for the four-step passes).
    // `tables`: the ahead-of-time form needs the sub-plan's column twiddles -- checked on the complex routes, a given on the real ones.
    // `rtc_ok`: hiprtc can build the kernel of this pass for the recipe.
    bool rows = false, tables = true;
    bool (*rtc_ok)(int, const JitCfg &) = jit_fourstep_ok;
    switch (pass) {
        case FS_CPX_1: case FS_CPX_2: tables = !c.twp_col.re.empty(); break;
        case FS_DCT4_2: tables = !c.twp_col.re.empty(); rtc_ok = jit_rfsi_ok; break;
        case FS_HALF_2: case FS_DCT2_2: break;
        case FS_C2R_1: case FS_DCT3_1: rtc_ok = jit_rfsi_ok; break;
        case FS_REAL_1: rows = true; rtc_ok = jit_rfs1_ok; break;
        case FS_C2R_LAST: rows = true; rtc_ok = jit_col_ok; break;
    }
    const JitCfg &recipe = rows ? c.jitcfg : c.fs_jitcfg;
    FsPlan p;
    p.pass = pass; p.F = F; p.sub = sub;
    if (fourstep_supported(F) && tables) {
        p.how = FS_AOT; p.twp = rows ? &DevConfig::twp : &DevConfig::twp_col;
        p.wide = (pass == FS_CPX_1 || pass == FS_CPX_2) && fourstep_wide(dtype, pass, F) && !c.twp_col_w.re.empty();
    } else if ((rows ? c.jit : c.fs_jit) && rtc_ok(dtype, recipe)) {
        p.how = FS_RTC; p.recipe = &recipe; p.twp = rows ? &DevConfig::twp : &DevConfig::twp_fs;
    }
    return p;
}
// Launches a planned pass on `a`, whose twiddle table (and wide flag) it sets.  kDeclined where the hiprtc launcher says unsupported.
template <typename T>
static int fs_launch(const FsPlan &p, bool inverse, RealArgs<T> &a, hipStream_t stream) {
    const DevTables *dt;
    const int rc = get_dev_tables(p.sub, &dt);
    if (rc) return rc;
    const DevConfig &d = dt->cfg[CFG_MAIN];
    a.wide = p.wide && !a.makhoul ? 1 : 0;      // (the fused DCT-IV first pass, makhoul = 2, exists in the staged E = 8 form only: launch_fourstep)
    a.twp = (const cpx<T> *)(a.wide ? d.twp_col_w : d.*p.twp);
    if (p.how == FS_RTC) return jit_rc(launch_jit_fourstep<T>(p.pass, inverse, *p.recipe, a, stream));
    return p.pass == FS_CPX_1 || p.pass == FS_CPX_2 ? launch_fourstep<T>(p.pass, p.F, inverse, a, stream) : launch_fourstep_real<T>(p.pass, p.F, a, stream);
}

// RealArgs of a four-step pass: zeroed (the struct's own defaults kept) but for the twiddles W_N^m = twhi[m >> logB] * twlo[m & (2^logB - 1)],
// N = cs_n, and the lane split (o, k1) = divmod(L / inner, k1n) of pow2_real.h's CS kernels
template <typename T>
static RealArgs<T> fs_args(const void *twlo, const void *twhi, int logB, int k1n, int f1, int64_t N) {
    RealArgs<T> a{};
    a.cs_twlo = (const cpx<T> *)twlo; a.cs_twhi = (const cpx<T> *)twhi; a.cs_logB = logB;
    a.cs_k1n = k1n; a.cs_f1 = f1; a.cs_n = (int)N;
    return a;
}

// Column four-step (pow2_real.h, CS kernels): a long STRIDED power-of-two lane, n = F1 * F2, as two passes
// of wide column tiles over a dense C-layout block [O][n][I] -- no transpose, no narrow tiles:
//   C2C      A: column C2C of length F1 over a = row / F2 (lanes (b, i): F2*I contiguous)  -> S[o][k1][b][i]
//            B: CS_C2C kernel of length F2 over b, twiddle on load, rows k1 + F1 k2            -> out
//   R2C      A: column R2C of length F1 (k1 = 0..F1/2); B: CS_R2C_2 kernel (Hermitian row map)   -> out rows 0..n/2
//   C2R      A: CS_C2R_1 kernel (Hermitian gather, inverse F2, conj twiddle) -> S; B: column C2R of length F1 -> out
// Cost: two reads + two writes of the array at 60-80 % of the HBM roofline each, against one pass of
// 16-32 byte row segments at 15-25 % (8192-long f32 lanes).
template <typename T>
static int col_split(const Problem &P, const void *d_in, void *d_out, const FftConfig &c, const DevConfig &d, hipStream_t stream) {
    const int64_t I = P.b.back().shape;
    const int64_t O = P.b.size() == 2 ? P.b[0].shape : 1;
    const int64_t sin_o = P.b.size() == 2 ? P.b[0].sin : 0, sout_o = P.b.size() == 2 ? P.b[0].sout : 0;
    const int F1 = c.cs_F1, F2 = c.cs_F2;
    const bool r2c = P.op == NDFFT_OP_R2C, c2r = P.op == NDFFT_OP_C2R, inv = P.op == NDFFT_OP_C2C_INV;
    const int K1 = (r2c || c2r) ? F1 / 2 + 1 : F1;
    // Column chunks: the intermediate of one chunk (K1*F2*C complex, <= 144 MiB) is written by stage A with
    // cache-allocating stores and re-read by stage B before much of it has left the 256 MiB Infinity Cache.
    // Measured (8192x8192 f32 R2C axis 0): one chunk 248 us, two chunks (136 MiB each) 212 us, three 228 us;
    // small chunks LOSE (32 MiB: 293 us, 8 MiB: 628 us): every chunk costs two launches of a few microseconds.
    // (round 6: odd chunks on a SECOND stream with a scratch array of their own, so that one chunk's launches drain under the other's work -- measured no better at any chunk size:
    //  cfg3-A 178 us (one stream, two chunks) against 184 (two streams, two chunks) / 183 (two streams, four chunks), cfg3-A' 193 against 219 / 192; profiles/r09/r09t_cs_two_streams_negative.txt)
    int64_t C = I;
    {
        const int64_t target = (int64_t)sw().cs_chunk_mb << 20;   // NDFFT_CS_CHUNK_MB (0 = one chunk)
        const int64_t per_col = (int64_t)K1 * F2 * (int64_t)sizeof(cpx<T>);
        if (target > 0 && O == 1 && per_col * I > target) {   // equal chunks, a multiple of 64 columns each
            const int64_t nchunk = (per_col * I + target - 1) / target;
            C = std::max<int64_t>(64, (((I + nchunk - 1) / nchunk) + 63) & ~(int64_t)63);
        }
        if (C > I) C = I;
    }
    const bool chunked = C < I;
    // Row pitch of the intermediate: C, dense rows.  It is OUR array, so its rows need not sit a power of two apart: tools/colprobe.hip
    // (profiles/r05/r05a_colprobe.txt) reads 256-byte segments 8192 rows deep at 0.55 of 8 TB/s when the rows are 32 KiB apart and
    // at 0.85 when they are 32 KiB + 512 B apart (writes 0.33 -> 0.70): a power-of-two pitch keeps every row of a column tile on
    // the same few HBM channels.  But padded rows measured on cfg3-A / cfg3-A' (profiles/r05/r05a_cs_pad_abab.txt): 0 / 256 / 512 / 1024 B all within 200-207 us: no effect, off
    const int64_t Cp = C;                    // pitch of one (k1, b) row of the intermediate, in complex elements
    void *S;
    int rc = get_scratch(5, stream, (size_t)O * K1 * F2 * Cp * sizeof(cpx<T>), &S);
    if (rc) return rc;
    const DevTables *dt2;
    if ((rc = get_dev_tables(c.cs_sub2, &dt2))) return rc;
    const size_t ein = (op_in_cplx(P.op) ? 2 : 1) * sizeof(T), eout = (op_out_cplx(P.op) ? 2 : 1) * sizeof(T);
    for (int64_t c0 = 0; c0 < I; c0 += C) {
        const int64_t Cc = std::min(C, I - c0);
        const char *in_c = (const char *)d_in + (size_t)c0 * ein;
        char *out_c = (char *)d_out + (size_t)c0 * eout;
        RealArgs<T> a = fs_args<T>(d.cs_twlo, d.cs_twhi, c.cs_logB, K1, F1, P.plan->n);
        a.nlanes = O * K1 * Cc;
        a.n = F2; a.F = F2; a.n_in = F2; a.n_out = F2; a.scale = (T)P.scale;
        a.twp = (const cpx<T> *)dt2->cfg[CFG_MAIN].twp_col;
        a.inner = Cc;
        a.cs_outer_in = sin_o; a.cs_outer_out = sout_o; a.cs_pitch = I;
        Problem Q;
        Q.plan = c.cs_sub1; Q.nlanes = O * F2 * Cc; Q.scale = 1.0; Q.no_xcd_map = 1;
        if (!c2r) {
            // A: column transform of length F1 over a = row / F2; lanes (b, i)
            Q.op = P.op; Q.xlen = F1; Q.ylen = K1; Q.xs = (int64_t)F2 * I; Q.ys = (int64_t)F2 * Cp;
            // (stream_in: the caller's array is read once and must not push the intermediate out of the Infinity Cache -- round 5, A-B-A-B on cfg3-A:
            //  198-201 -> 188.5-191 us; the C2R form's first stage below: 225 -> 220 us; profiles/r08/r08r_cs_stage_nt_abab.txt)
            Q.keep_out = chunked; Q.stream_in = (int)NDFFT_DEV_INT("NDFFT_CSA_NT", 1);
            if (chunked) { Q.b.push_back({(int64_t)F2, I, Cp}); Q.b.push_back({Cc, 1, 1}); }   // (b, i) as two batch dimensions: the intermediate's rows are not back to back
            else {
                if (O > 1) Q.b.push_back({O, sin_o, (int64_t)K1 * F2 * I});
                Q.b.push_back({(int64_t)F2 * I, 1, 1});
            }
            if ((rc = dispatch(Q, in_c, S, stream))) return rc;
            // B: twiddle on load, length F2 over b, rows k1 + F1 k2 (R2C: Hermitian row map)
            a.in = S; a.out = out_c;
            a.outer_in = (int64_t)F2 * Cp; a.outer_out = 0; a.elem_in = Cp; a.elem_out = (int64_t)F1 * I;
            if ((rc = launch_colsplit<T>(r2c ? CS_R2C_2 : CS_C2C, inv, a, stream))) return rc;
        } else {
            // A: Hermitian gather, inverse of length F2 over k2, conj twiddle -> S[o][k1][b][i]
            a.in = in_c; a.out = S;
            a.outer_in = 0; a.outer_out = (int64_t)F2 * Cp; a.elem_in = I; a.elem_out = Cp;
            a.stream_in = (int)NDFFT_DEV_INT("NDFFT_CS3_NT", 1);
            if ((rc = launch_colsplit<T>(CS_C2R_1, true, a, stream))) return rc;
            a.stream_in = 0;
            // B: column C2R of length F1 over k1
            Q.op = NDFFT_OP_C2R; Q.xlen = K1; Q.ylen = F1; Q.xs = (int64_t)F2 * Cp; Q.ys = (int64_t)F2 * I;
            if (chunked) { Q.b.push_back({(int64_t)F2, Cp, I}); Q.b.push_back({Cc, 1, 1}); }
            else {
                if (O > 1) Q.b.push_back({O, (int64_t)K1 * F2 * I, sout_o});
                Q.b.push_back({(int64_t)F2 * I, 1, 1});
            }
            if ((rc = dispatch(Q, S, out_c, stream))) return rc;
        }
    }
    set_last_path("col_split");
    return NDFFT_OK;
}

// Pitch padding of the four-step routes' intermediates (round 5).  Pass 2 reads the intermediate as column tiles: 128-byte rows one pitch apart.  With the natural
// power-of-two pitch (256 x 65536 c128: 4096 B) the rows of a tile fall on few HBM channels; 128 bytes more per row and a copy of that shape runs 6.5 % faster
// (9 % with streaming LDS-DMA loads; + 512 B: 3.7 %, + 1 KiB: slower -- tools/ldsdma_probe.hip `fs2`, profiles/r08/r08j_fs2_pitch.txt).  The real four-step's
// forward intermediate always had such a pitch (N1/2 + 1 rounded up to whole lines).  In the product the gain is small: nddct4 64 x 262144 f64 165 -> 157 us,
// 32 x 2^20 c64 291 -> 281-288 us, 256 x 65536 c128 204 -> 201-204 us (profiles/r08/r08k_longlanes_pad.txt) -- the passes already run at the copy rate of
// their tile shapes (two passes of 537 MB at 5.3-5.7 TB/s = 195 us for the c128 case).  Elements of type cpx<T>.
template <typename T> static int fs_pad_elems() { return (int)(NDFFT_DEV_INT("NDFFT_FS_PAD", 128) / (long)sizeof(cpx<T>)); }

// Four-step complex FFT of length F = F1*F2 on L lanes (zin / zout: lane pitches in elements).
// zin may equal zout.  Sub-FFTs run through dispatch() on the row kernels.
template <typename T>
static int big_fft(const FftConfig &c, const DevConfig &d, const cpx<T> *zin, int64_t pitch_in, cpx<T> *zout, int64_t pitch_out,
                   int64_t L, bool inverse, T scale, hipStream_t stream) {
    if (c.bigblue) {
        // Bluestein over global memory: two FFT_M through dispatch() (pow2 row kernel, or its own four-step for
        // M > 16384 -- which uses scratch slots 2 / 3, hence 6 / 7 here) between three elementwise stages
        const int Fl = c.F, M = c.M;
        void *a1, *a2;
        int rcb;
        if ((rcb = get_scratch(6, stream, (size_t)L * M * sizeof(cpx<T>), &a1))) return rcb;
        if ((rcb = get_scratch(7, stream, (size_t)L * M * sizeof(cpx<T>), &a2))) return rcb;
        const cpx<T> *chirp = (const cpx<T> *)d.chirp, *bhat = (const cpx<T> *)d.bhat;
        if ((rcb = launch_blue_stage<T>(0, (cpx<T> *)a1, M, zin, pitch_in, L, Fl, M, chirp, bhat, inverse ? 1 : 0, (T)1, stream))) return rcb;
        Problem Q;
        Q.plan = c.sub1; Q.op = NDFFT_OP_C2C_FWD; Q.xlen = Q.ylen = M; Q.xs = Q.ys = 1; Q.nlanes = L; Q.scale = 1.0;
        Q.b.push_back({L, (int64_t)M, (int64_t)M});
        if ((rcb = dispatch(Q, a1, a2, stream))) return rcb;
        if ((rcb = launch_blue_stage<T>(1, (cpx<T> *)a2, M, (const cpx<T> *)a2, M, L, Fl, M, chirp, bhat, 0, (T)1, stream))) return rcb;
        if ((rcb = dispatch(Q, a2, a1, stream))) return rcb;
        return launch_blue_stage<T>(2, zout, pitch_out, (const cpx<T> *)a1, M, L, Fl, M, chirp, bhat, inverse ? 1 : 0, inverse ? scale : (T)1, stream);
    }
    const int F1 = c.F1, F2 = c.F2;
    const int64_t F = (int64_t)F1 * F2;
    const int esz = (int)sizeof(cpx<T>);
    void *s1, *s2;
    int rc;
    const int64_t K1p = F1 + fs_pad_elems<T>();       // pitch of the two-pass intermediate s1[n2][k1]
    if ((rc = get_scratch(2, stream, (size_t)(L * std::max<int64_t>(F, (int64_t)F2 * K1p)) * esz, &s1))) return rc;
    // Two-pass form, no transpose launch, when both factors have a column kernel (powers of two, 64..1024):
    //   (1) length-F1 FFTs over the strided n1 axis, column load, stored TRANSPOSED as s1[n2][k1] (row store)
    //   (2) length-F2 FFTs over n2 of s1 (stride F1, adjacent k1 contiguous), twiddle W_F^(n2 k1) on load, stored at
    //       k1 + F1 k2 = natural order.   256 x 65536 c128: 317 us (three passes) -> see DESIGN.md section 3.5
    // (round 6: a smooth NON-power-of-two factor runs the same two passes on kernels specialised with hiprtc -- jit.hip: launch_jit_fourstep -- instead of the six-pass transpose route)
    const FsPlan p1 = fs_plan(FS_CPX_1, F1, c.sub1, dtype_of<T>()), p2 = fs_plan(FS_CPX_2, F2, c.sub2, dtype_of<T>());
    // (a declined hiprtc pass falls through to the forms below: only the scratch s1 has been written, zout is untouched)
    if (p1 && p2 && fourstep2_enabled()) {
        RealArgs<T> a = fs_args<T>(d.twlo, d.twhi, c.logB, 1, F1, F);
        // (used by the half-line tiles only, F = 1024 f32 -- pow2_real.h; 32 x 2^20 c64: 403 -> 354 us, profiles/r06)
        a.xcd_chunk = (int)NDFFT_DEV_INT("NDFFT_FS_XCD_CHUNK", 32);
        // pass 1: lanes (l, n2)
        a.in = zin; a.out = s1; a.nlanes = L * F2; a.n = F1; a.F = F1; a.n_in = F1; a.n_out = F1; a.scale = (T)1;
        a.inner = F2; a.outer_in = pitch_in; a.elem_in = F2; a.pitch_out = K1p;
        // c128 (the lane-fastest kernels): the caller's array is read once -> streaming loads; the intermediate is re-read by pass 2 -> cache-allocating stores.
        // A-B-A-B (profiles/r08/r08s_fourstep_pass1_policy_abab.txt): 256 x 65536 203 -> 197 us, 16 x 2^20 260 -> 248 us; either one alone is neutral or worse
        // (keep alone: 213 us); c64 (staged kernels) 285 -> 291 us with the streaming loads: off there
        a.stream_in = (int)NDFFT_DEV_INT("NDFFT_FS_P1_NT", sizeof(T) == 8 ? 1 : 0); a.keep_out = (int)NDFFT_DEV_INT("NDFFT_FS_KEEP", sizeof(T) == 8 ? 1 : 0);
        rc = fs_launch<T>(p1, inverse, a, stream);
        if (rc == NDFFT_OK) {
            a.stream_in = 0; a.keep_out = 0;
            // pass 2: lanes (l, k1)
            a.in = s1; a.out = zout; a.nlanes = L * F1; a.n = F2; a.F = F2; a.n_in = F2; a.n_out = F2; a.scale = scale;
            a.inner = F1; a.outer_in = (int64_t)F2 * K1p; a.outer_out = pitch_out; a.elem_in = K1p; a.elem_out = F1; a.pitch_out = 0;
            rc = fs_launch<T>(p2, inverse, a, stream);
        }
        if (rc != kDeclined) return rc;
    }
    if ((rc = get_scratch(3, stream, (size_t)(L * F) * esz, &s2))) return rc;
    // Fused three-pass form when both halves run on the register kernels:
    //   (1) length-F1 FFTs IN PLACE of the layout, on the strided n1 axis, by the column-tile kernels
    //   (2) length-F2 row FFTs whose load multiplies by the four-step twiddle W_F^{n2 k1}
    //   (3) one transpose into natural order
    {
        const bool row2 = c.sub2->cfg[CFG_MAIN].pow2;
        const int col_lanes = std::is_same<T, float>::value ? pow2_real_col_lanes<float>(F1, 0) : pow2_real_col_lanes<double>(F1, 0);
        const int nar_lanes = std::is_same<T, float>::value ? pow2_real_narrow_lanes<float>(F1) : pow2_real_narrow_lanes<double>(F1);
        const bool col1 = !c.sub1->cfg[CFG_MAIN].twp_col.re.empty() && F2 >= 8 && col_lanes > 0;
        const bool nar1 = !c.sub1->cfg[CFG_MAIN].twp_narrow.re.empty() && F2 >= 64 && nar_lanes > 0;
        if (row2 && (col1 || nar1)) {
            Problem Q;
            Q.plan = c.sub1; Q.op = inverse ? NDFFT_OP_C2C_INV : NDFFT_OP_C2C_FWD;
            Q.xlen = Q.ylen = F1; Q.xs = Q.ys = F2; Q.nlanes = L * F2; Q.scale = 1.0;
            if (L > 1) Q.b.push_back({L, pitch_in, F});
            Q.b.push_back({(int64_t)F2, 1, 1});
            if ((rc = dispatch(Q, zin, s1, stream))) return rc;
            const DevTables *dt2;
            if ((rc = get_dev_tables(c.sub2, &dt2))) return rc;
            Pow2Args a;
            a.in = s1; a.out = s2; a.nlanes = L * F1; a.pitch_in = F2; a.pitch_out = F2;
            a.inverse = inverse; a.scale = (double)scale; a.twp = dt2->cfg[CFG_MAIN].twp;
            a.twlo = d.twlo; a.twhi = d.twhi; a.logB = c.logB; a.f1 = F1;
            if ((rc = launch_pow2(c.sub2->dtype, F2, a, stream))) return rc;
            return transpose_batched(s2, zout, L, F1, F2, F2, F1, F, pitch_out, esz, stream);
        }
    }
    // x[n1][n2] -> s1[n2][n1]
    if ((rc = transpose_batched(zin, s1, L, F1, F2, F2, F1, pitch_in, F, esz, stream))) return rc;
    Problem Q;
    Q.plan = c.sub1; Q.op = inverse ? NDFFT_OP_C2C_INV : NDFFT_OP_C2C_FWD;
    Q.xlen = Q.ylen = F1; Q.xs = Q.ys = 1; Q.nlanes = L * F2; Q.scale = 1.0;
    Q.b.push_back({L * F2, (int64_t)F1, (int64_t)F1});
    if ((rc = dispatch(Q, s1, s2, stream))) return rc;
    if ((rc = launch_big_twiddle<T>((cpx<T> *)s2, L, F1, F2, (const cpx<T> *)d.twlo, (const cpx<T> *)d.twhi, c.logB, inverse ? 1 : 0, scale, stream))) return rc;
    // s2[n2][k1] -> s1[k1][n2]
    if ((rc = transpose_batched(s2, s1, L, F2, F1, F1, F2, F, F, esz, stream))) return rc;
    Q.plan = c.sub2; Q.xlen = Q.ylen = F2; Q.nlanes = L * F1;
    Q.b.clear(); Q.b.push_back({L * F1, (int64_t)F2, (int64_t)F2});
    if ((rc = dispatch(Q, s1, s2, stream))) return rc;
    // s2[k1][k2] -> out[k2][k1]  (flat index k1 + F1 k2)
    return transpose_batched(s2, zout, L, F1, F2, F2, F1, F, pitch_out, esz, stream);
}

// REAL four-step for long contiguous real-data lanes, n = N1 * N2 a power of two (plan.hip: add_real_fourstep), R2C and DCT-II:
//   (1) real FFTs of length N1 over the strided index n1 of x[n1 N2 + n2] (DCT-II: of Makhoul's permutation of x, gathered by the load),
//       half spectrum stored transposed, s[lane][n2][k1], k1 = 0..N1/2
//   (2) complex FFTs of length N2 over n2 with the twiddle W_n^(n2 k1) fused into the load; X[k1 + N1 k2] and, for the other half of every
//       lane, conj at the mirrored index -- the half spectrum 0..n/2 exactly once; DCT-II multiplies by e^(-i pi k / 2n) and writes y[k], y[n-k]
// Two passes and an intermediate of n/2 + N2 complex per lane; the packed complex four-step needs a split pass (and a Makhoul pass) around its two.
// gop = G_DCT1 (round 5): the lane is the even extension of the caller's n = N1 N2 / 2 + 1 points (pass 1 gathers it: makhoul = 3) and pass 2 stores y[k] = Re X[k] / 2 times the
// pre-scale (src/lib.rs:688-698) for k = 0 .. n - 1 -- c / d are the DCT1 slot's tables then.
template <typename T>
static int real_fourstep(const Problem &P, int gop, const FftConfig &c, const DevConfig &d, const void *d_in, void *d_out, int64_t pin, int64_t pout, hipStream_t stream) {
    const int N1 = c.rfs_N1, N2 = c.rfs_N2;
    const bool dct1 = gop == G_DCT1;
    // k1 = 0..N1/2 of the intermediate on a pitch of whole 128-byte lines (the tiles of pass 2 are 128 bytes of adjacent k1 wide: with the
    // natural pitch N1/2 + 1 every tile row would straddle two lines shared with a tile on another XCD)
    const int K = (N1 / 2 + 1 + (int)(128 / sizeof(cpx<T>)) - 1) & ~((int)(128 / sizeof(cpx<T>)) - 1);
    const int64_t n = (int64_t)N1 * N2, B = P.nlanes;
    const DevTables *dt1;
    int rc;
    // (round 6: a factor that is not a power of two runs its pass on a kernel specialised with hiprtc -- plan.hip: add_real_fourstep_smooth; declined before
    //  anything is launched when that is not to be had: the caller falls back to the packed route)
    const FsPlan p1 = fs_plan(FS_REAL_1, N1 / 2, c.rfs_sub1, dtype_of<T>()), p2 = fs_plan(gop == G_DCT2_EVEN ? FS_DCT2_2 : FS_HALF_2, N2, c.rfs_sub2, dtype_of<T>());
    if (!p1 || !p2) return kDeclined;
    if ((rc = get_dev_tables(c.rfs_sub1, &dt1))) return rc;
    void *s1;
    if ((rc = get_scratch(4, stream, (size_t)(B * N2 * K) * sizeof(cpx<T>), &s1))) return rc;
    RealArgs<T> a = fs_args<T>(d.rfs_twlo, d.rfs_twhi, c.rfs_logB, 1, N1, n);
    // pass 1: lanes (l, n2), real input
    a.in = d_in; a.out = s1; a.nlanes = B * N2; a.n = N1; a.F = N1 / 2; a.n_in = N1; a.n_out = N1 / 2 + 1; a.scale = (T)1;
    a.inner = N2; a.outer_in = pin; a.elem_in = N2; a.pitch_out = K;
    a.aux1 = (const cpx<T> *)dt1->cfg[CFG_MAIN].aux1;
    a.makhoul = gop == G_DCT2_EVEN ? 1 : dct1 ? 3 : 0;
    // streaming loads of the caller's lane in pass 1: R2C re-read 123.5 -> 118 us (HBM-sourced unchanged); not for DCT-II, whose mirror tiles share every line
    // (134 -> 144 us) -- profiles/r08/r08t_real_fourstep_policy_abab.txt
    // (round 6, A-B-A-B on the developer build, profiles/r09/r09l_rfs_p1_nt_abab.txt: with the lane coming from HBM streaming loads LOSE -- 122 against 119 us --, with a re-read,
    //  cache-resident lane they win -- 113 against 118 us: a resident lane read with nt loads is not re-allocated and leaves the cache to the intermediate.  So the residency
    //  model decides: streaming loads only for an input it expects IN the cache.  NDFFT_RFS_P1_NT = 0 / 1 (developer build) forces one form, 2 = the model.)
    {
        const long knob = NDFFT_DEV_INT("NDFFT_RFS_P1_NT", 2);
        const size_t es = sizeof(T);
        const bool resident = row_load_policy(d_in, (size_t)B * (dct1 ? (size_t)(n / 2 + 1) : (size_t)n) * es, d_out, (size_t)B * (size_t)(gop == G_R2C_EVEN ? (n / 2 + 1) * 2 : dct1 ? n / 2 + 1 : n) * es) == 0;
        a.stream_in = (gop == G_DCT2_EVEN || dct1) ? 0 : (knob == 2 ? (resident ? 1 : 0) : (int)knob);     // (DCT-I reads every element twice, through its own tile and the mirrored one)
    }
    if ((rc = fs_launch<T>(p1, false, a, stream))) return rc;
    a.stream_in = 0;
    // pass 2: lanes (l, k1)
    a.makhoul = dct1 ? 3 : 0;                        // (3: real outputs Re X[k] a.scale)
    a.keep_out = 1;                                  // plain stores at the lines the mirrored rows share
    a.xcd_chunk = (int)NDFFT_DEV_INT("NDFFT_RFS_XCD_CHUNK", 8);
    a.in = s1; a.out = d_out; a.nlanes = B * K; a.n = N2; a.F = N2; a.n_in = N2; a.n_out = N2; a.scale = dct1 ? (T)(0.5 * P.scale) : (T)P.scale;
    a.inner = K; a.outer_in = (int64_t)N2 * K; a.outer_out = pout; a.elem_in = K; a.pitch_out = 0;
    a.aux1 = nullptr; a.aux2 = (const cpx<T> *)d.aux2;
    if (gop == G_DCT2_EVEN && NDFFT_DEV_INT("NDFFT_RFS_FACTORED", 1)) { a.fc1 = (const cpx<T> *)d.rfs_c1; a.fc2 = (const cpx<T> *)d.rfs_c2; }
    return fs_launch<T>(p2, false, a, stream);
}

// The inverse direction of the real four-step, C2R and DCT-III:
//   (1) for k1 = 0..N1/2: the elements Xh[k1 + N1 k2] of the Hermitian extension (DCT-III: V[k] built from x[k], x[n-k]), unnormalised inverse FFT of
//       length N2 over k2, times W_n^(-n2 k1), stored as s[lane][k1][n2]
//   (2) column C2R of length N1 over k1 for every n2 (the ordinary column kernel: adjacent n2 contiguous on both sides) -> x[n1 N2 + n2]
//       (DCT-III: written through the inverse of Makhoul's permutation)
template <typename T>
static int real_fourstep_inv(const Problem &P, int gop, const FftConfig &c, const DevConfig &d, const void *d_in, void *d_out, int64_t pin, int64_t pout, hipStream_t stream) {
    const int N1 = c.rfs_N1, N2 = c.rfs_N2, Kx = N1 / 2 + 1;
    const int Kp = (Kx + (int)(128 / sizeof(cpx<T>)) - 1) & ~((int)(128 / sizeof(cpx<T>)) - 1);   // lanes per o, padded: every tile starts on a 128-byte line of the input
    const int64_t n = (int64_t)N1 * N2, B = P.nlanes;
    int rc;
    // (round 6: N2 not a power of two -> pass 1 on the hiprtc form of the lane-fastest kernel; N1 / 2 not a power of two -> pass 2 through dispatch(): the general column C2R kernel, hiprtc too)
    const FsPlan p1 = fs_plan(gop == G_DCT3_EVEN ? FS_DCT3_1 : FS_C2R_1, N2, c.rfs_sub2, dtype_of<T>());
    if (!p1) return kDeclined;
    // DCT-III writes its outputs through the inverse of Makhoul's permutation in the LAST pass: only the column-tile kernels do that (RealArgs::makhoul), and dispatch() may
    // pick another kernel for a length that is not a power of two (a small call runs the generic kernel) -- so DCT-III needs the ahead-of-time last pass
    // ... or the hiprtc column tile of that length, launched HERE.  C2R takes the tile pass only in its ahead-of-time form.
    const FsPlan last = gop == G_DCT3_EVEN || fourstep_supported(N1 / 2) ? fs_plan(FS_C2R_LAST, N1 / 2, c.rfs_sub1, dtype_of<T>()) : FsPlan();
    if (gop == G_DCT3_EVEN && !last) return kDeclined;
    void *s1;
    // (no pitch padding here: with + 128 B per row ndifft_r2c 64 x 262144 f64 measured 112 -> 118 us, nddct3 unchanged -- profiles/r08/r08k_longlanes_pad.txt)
    const int64_t N2p = N2;                          // pitch of the intermediate s[k1][n2]
    if ((rc = get_scratch(4, stream, (size_t)(B * Kx * N2p) * sizeof(cpx<T>), &s1))) return rc;
    RealArgs<T> a = fs_args<T>(d.rfs_twlo, d.rfs_twhi, c.rfs_logB, Kx, N1, n);
    a.aux2 = (const cpx<T> *)d.aux2;
    a.in = d_in; a.out = s1; a.nlanes = B * Kp; a.n = N2; a.F = N2; a.n_in = N2; a.n_out = N2; a.scale = (T)P.scale;
    a.inner = Kp; a.outer_in = pin; a.elem_in = N1; a.pitch_out = N2p;
    // runs of consecutive tiles per XCD: the mirrored index N1 - k1 is shifted by one element against the tile grid (and DCT-III's real rows are
    // half lines), so neighbouring tiles share every line
    a.xcd_chunk = (int)NDFFT_DEV_INT("NDFFT_RFS_XCD_CHUNK", 8);
    a.stream_in = (int)NDFFT_DEV_INT("NDFFT_RFSI_P1_NT", 0);      // (measured: ndifft_r2c re-read 112 -> 125 us with streaming loads of the half spectrum: off)
    if (gop == G_DCT3_EVEN && NDFFT_DEV_INT("NDFFT_RFS_FACTORED", 1)) { a.fc1 = (const cpx<T> *)d.rfs_c1; a.fc2 = (const cpx<T> *)d.rfs_c2; }
    if ((rc = fs_launch<T>(p1, false, a, stream))) return rc;
    a.stream_in = 0;
    if (last.how == FS_RTC || (last.how == FS_AOT && sw().rfs_c2r_tile)) {   // the column C2R kernel on 128-byte tiles (0: the general column kernel through dispatch())
        const DevTables *dt1;
        if ((rc = get_dev_tables(c.rfs_sub1, &dt1))) return rc;
        a.xcd_chunk = 0; a.keep_out = 0; a.fc1 = nullptr; a.fc2 = nullptr;
        a.in = s1; a.out = d_out; a.nlanes = B * N2; a.n = N1; a.F = N1 / 2; a.n_in = Kx; a.n_out = N1; a.scale = (T)1;
        a.inner = N2; a.outer_in = (int64_t)Kx * N2p; a.outer_out = pout; a.elem_in = N2p; a.elem_out = N2; a.pitch_in = 0; a.pitch_out = 0;
        a.aux1 = (const cpx<T> *)dt1->cfg[CFG_MAIN].aux1;
        a.makhoul = gop == G_DCT3_EVEN ? 1 : 0;
        return fs_launch<T>(last, false, a, stream);
    }
    Problem Q;
    Q.plan = c.rfs_sub1; Q.op = NDFFT_OP_C2R; Q.xlen = Kx; Q.ylen = N1; Q.xs = N2p; Q.ys = N2; Q.nlanes = B * N2; Q.scale = 1.0;
    if (B > 1) Q.b.push_back({B, (int64_t)Kx * N2p, pout});
    Q.b.push_back({(int64_t)N2, 1, 1});
    Q.no_xcd_map = 1; Q.makhoul_out = gop == G_DCT3_EVEN ? 1 : 0;
    return dispatch(Q, s1, d_out, stream);
}

// DCT-IV of a long even lane, n = 2 F, F = F1 * F2 powers of two: the complex four-step of length F with the fold z[j] = (x[2j] + i x[n-1-2j]) s w_j built by
// pass 1's load and the outputs y[2k] = Re(Z[k] c_k), y[n-1-2k] = -Im(Z[k] c_k) written by pass 2's store -- two passes instead of four.
template <typename T>
static int dct4_fourstep(const Problem &P, const FftConfig &c, const DevConfig &d, const void *d_in, void *d_out, int64_t pin, int64_t pout, hipStream_t stream, const FsPlan &p1, const FsPlan &p2) {
    const int F1 = c.F1, F2 = c.F2;
    const int64_t F = (int64_t)F1 * F2, B = P.nlanes;
    int rc;
    void *s1;
    const int64_t K1p = F1 + fs_pad_elems<T>();      // pitch of the intermediate s1[n2][k1] (fs_pad_elems)
    if ((rc = get_scratch(2, stream, (size_t)(B * F2 * K1p) * sizeof(cpx<T>), &s1))) return rc;
    RealArgs<T> a = fs_args<T>(d.twlo, d.twhi, c.logB, 1, F1, 2 * F);
    a.aux1 = (const cpx<T> *)d.aux1; a.aux2 = (const cpx<T> *)d.aux2;
    // pass 1: lanes (l, n2) of the REAL input
    a.in = d_in; a.out = s1; a.nlanes = B * F2; a.n = F1; a.F = F1; a.n_in = F1; a.n_out = F1; a.scale = (T)P.scale;
    a.inner = F2; a.outer_in = pin; a.elem_in = F2; a.pitch_out = K1p;
    a.makhoul = 2;
    // pass 1: streaming loads of the caller's lane, cache-allocating stores of the intermediate (the staged ROWOUT store ignored keep_out until round 5):
    // nddct4 64 x 262144 f64 157.6 -> 153.3 (stores) -> 148-150 us (both)
    a.stream_in = (int)NDFFT_DEV_INT("NDFFT_DCT4_P1_NT", 1); a.keep_out = (int)NDFFT_DEV_INT("NDFFT_DCT4_KEEP", 1);
    if ((rc = fs_launch<T>(p1, false, a, stream))) return rc;
    a.stream_in = 0;
    // pass 2: lanes (l, k1), real output
    a.makhoul = 0; a.keep_out = 0;
    a.in = s1; a.out = d_out; a.nlanes = B * F1; a.n = F2; a.F = F2; a.n_in = F2; a.n_out = F2; a.scale = (T)1;
    a.inner = F1; a.outer_in = (int64_t)F2 * K1p; a.outer_out = pout; a.elem_in = K1p; a.elem_out = 0; a.pitch_out = 0;
    return fs_launch<T>(p2, false, a, stream);
}

// contiguous lanes whose inner FFT does not fit one workgroup's LDS
template <typename T>
static int dispatch_big(const Problem &P, const void *d_in, void *d_out, const DevTables &dt, hipStream_t stream) {
    const ndfft_plan *plan = P.plan;
    int slot;
    const int gop = gen_op_of(P.op, (int)plan->n, &slot);
    const FftConfig &c = plan->cfg[slot];
    const DevConfig &d = dt.cfg[slot];
    const int64_t pin = P.b.empty() ? P.xlen : P.b[0].sin, pout = P.b.empty() ? P.ylen : P.b[0].sout;
    if (gop == G_C2C_FWD || gop == G_C2C_INV) {
        int rc0 = big_fft<T>(c, d, (const cpx<T> *)d_in, pin, (cpx<T> *)d_out, pout, P.nlanes, gop == G_C2C_INV, (T)P.scale, stream);
        set_last_path(c.bigblue ? "blue_global" : "four_step");
        return rc0;
    }
    // (a plan whose factors are not powers of two has the forward ops only, and its passes need hiprtc: real_fourstep declines before anything is launched
    //  when that is not to be had -> packed route below)
    const bool rfs_smooth = c.rfs && (((c.rfs_N1 & (c.rfs_N1 - 1)) != 0) || ((c.rfs_N2 & (c.rfs_N2 - 1)) != 0));
    const int rfs_on = real_fourstep_enabled(), rfs_ops = (rfs_on == 2 ? (c.rfs_ops & 16 ? 16 : 15) : (rfs_on ? c.rfs_ops : 0)) & (rfs_smooth ? c.rfs_ops : 31);
    int rc = kDeclined;
    if (c.rfs && ((gop == G_DCT1 && (rfs_ops & 16)) || (gop == G_DCT2_EVEN && (rfs_ops & 4)) || (gop == G_R2C_EVEN && P.scale == 1.0 && (rfs_ops & 1)))) {
        rc = real_fourstep<T>(P, gop, c, d, d_in, d_out, pin, pout, stream);
    } else if (gop == G_DCT4_EVEN && rfs_on && c.big && !c.bigblue && fourstep2_enabled()) {
        // (round 6: a factor that is not a power of two on the hiprtc forms of the same two kernels -- pass 1 the staged ROWOUT kernel, pass 2 the lane-fastest one, whole rounds)
        const FsPlan p1 = fs_plan(FS_CPX_1, c.F1, c.sub1, dtype_of<T>()), p2 = p1 ? fs_plan(FS_DCT4_2, c.F2, c.sub2, dtype_of<T>()) : FsPlan();
        if (p2) rc = dct4_fourstep<T>(P, c, d, d_in, d_out, pin, pout, stream, p1, p2);
    } else if (c.rfs && ((gop == G_C2R_EVEN && (rfs_ops & 2)) || (gop == G_DCT3_EVEN && (rfs_ops & 8)))) {
        rc = real_fourstep_inv<T>(P, gop, c, d, d_in, d_out, pin, pout, stream);
    }
    if (rc != kDeclined) {
        set_last_path("real_four_step");
        return rc;
    }
    // packed: PRE pass -> complex four-step of length F -> POST pass
    RealArgs<T> a{};
    a.in = d_in; a.out = d_out; a.nlanes = P.nlanes; a.pitch_in = pin; a.pitch_out = pout;
    a.n = (int)plan->n; a.F = c.F; a.n_in = (int)P.xlen; a.n_out = (int)P.ylen; a.scale = (T)P.scale;
    a.aux1 = (const cpx<T> *)d.aux1; a.aux2 = (const cpx<T> *)d.aux2;
    void *z;
    if ((rc = get_scratch(4, stream, (size_t)(P.nlanes * c.F) * sizeof(cpx<T>), &z))) return rc;
    // Two of the ops need only ONE of the elementwise passes over global memory (round 3):
    //   R2C, even n: the PRE fold is z[i] = (x[2i], x[2i+1]) -- the raw real lane read as complex.  The FFT takes the input array itself.
    //   C2R, even n: the POST is x[2k] = Re, x[2k+1] = -Im of the forward FFT of conj(Zt) -- i.e. the inverse-by-conjugation of Zt written
    //                into the real output lane read as complex.  PRE emits Zt, the FFT runs as an inverse and stores the result itself.
    const bool cplx_view_ok = [&] {   // a real lane can be addressed as complex elements: even pitch, complex-aligned base
        const void *p = gop == G_R2C_EVEN ? d_in : (const void *)d_out;
        const int64_t pitch = gop == G_R2C_EVEN ? pin : pout;
        return pitch % 2 == 0 && (uintptr_t)p % sizeof(cpx<T>) == 0;
    }();
    if (gop == G_R2C_EVEN && cplx_view_ok) {
        if ((rc = big_fft<T>(c, d, (const cpx<T> *)d_in, pin / 2, (cpx<T> *)z, c.F, P.nlanes, false, (T)1, stream))) return rc;
        rc = launch_big_post<T>(gop, a, (const cpx<T> *)z, stream);
    } else if (gop == G_C2R_EVEN && cplx_view_ok) {
        if ((rc = launch_big_pre<T>(gop, a, (cpx<T> *)z, stream, 1))) return rc;
        rc = big_fft<T>(c, d, (const cpx<T> *)z, c.F, (cpx<T> *)d_out, pout / 2, P.nlanes, true, (T)1, stream);
    } else {
        if ((rc = launch_big_pre<T>(gop, a, (cpx<T> *)z, stream))) return rc;
        if ((rc = big_fft<T>(c, d, (const cpx<T> *)z, c.F, (cpx<T> *)z, c.F, P.nlanes, false, (T)1, stream))) return rc;
        rc = launch_big_post<T>(gop, a, (const cpx<T> *)z, stream);
    }
    set_last_path(c.bigblue ? "blue_global" : "four_step");
    return rc;
}

// Long lanes on a non-contiguous axis of a C-layout array, viewed as (outer, n, inner):
// transpose -> row transform on contiguous lanes -> transpose back.
static int dispatch_transposed(const Problem &P, const void *d_in, void *d_out, hipStream_t stream, int64_t outer,
                               int64_t inner, size_t ein, size_t eout) {
    const int64_t n_in = P.xlen, n_out = P.ylen;
    // scratch lanes are pitched to a multiple of 16 bytes so both transposes can use 16-byte accesses
    const int64_t p_in = (n_in + 3) & ~(int64_t)3, p_out = (n_out + 3) & ~(int64_t)3;
    void *s1, *s2;
    int rc;
    if ((rc = get_scratch(0, stream, (size_t)(outer * inner * p_in) * ein, &s1))) return rc;
    if ((rc = get_scratch(1, stream, (size_t)(outer * inner * p_out) * eout, &s2))) return rc;
    // in[o][j][i] -> s1[o][i][j]
    if ((rc = transpose_batched(d_in, s1, outer, n_in, inner, inner, p_in, n_in * inner, inner * p_in, (int)ein, stream))) return rc;
    Problem Q = P;
    Q.xs = Q.ys = 1;
    Q.b.clear();
    Q.b.push_back({outer * inner, p_in, p_out});
    if ((rc = dispatch(Q, s1, s2, stream))) return rc;
    // s2[o][i][k] -> out[o][k][i]
    return transpose_batched(s2, d_out, outer, inner, n_out, p_out, inner, inner * p_out, n_out * inner, (int)eout, stream);
}

// one dispatch(): what every route reads
struct Call {
    const Problem &P;
    const void *in; void *out; hipStream_t stream;
    const ndfft_plan *plan; const DevTables &dt;
    const Layout L;
    const int n;                     // handler length
    int slot, gop;                   // plan slot and kernel op of P.op (gen_op_of)
    Call(const Problem &P_, const void *in_, void *out_, hipStream_t s, const DevTables &dt_)
        : P(P_), in(in_), out(out_), stream(s), plan(P_.plan), dt(dt_), L(P_), n((int)P_.plan->n) { gop = gen_op_of(P.op, n, &slot); }
    bool f32() const { return plan->dtype == NDFFT_F32; }
};

// short dense power-of-two C2C lanes (n = 2..64): the LDS-free wavefront kernel -- coalesced 16-byte accesses and
// cross-lane shuffles (wave_kernel.h).  NDFFT_WAVE=0 keeps the older paths (parity tests cover both).
static int route_wave(const Call &k) {
    const DevConfig &d = k.dt.cfg[CFG_MAIN];
    if (!(k.plan->kind == NDFFT_KIND_C2C && wave_supported(k.n) && d.wave_tw && k.L.dense && (uintptr_t)k.in % 16 == 0 &&
          (uintptr_t)k.out % 16 == 0 && wave_enabled()))
        return kDeclined;
    WaveArgs a;
    a.in = k.in; a.out = k.out; a.total = k.P.nlanes * (int64_t)k.n;
    a.inverse = k.P.op == NDFFT_OP_C2C_INV; a.scale = k.P.scale; a.tw = d.wave_tw; a.xcd_chunk = 0;
    set_last_path("wave_reg");
    return launch_wave(k.plan->dtype, k.n, a, k.stream);
}

// the arguments of the thread-per-lane kernels (tiny, reg, regreal, tinymat)
static TinyArgs tiny_args(const Call &k, int inverse, const void *mat) {
    TinyArgs a;
    a.in = k.in; a.out = k.out; a.nlanes = k.P.nlanes; a.inverse = inverse; a.scale = k.P.scale; a.mat = mat;
    a.elem_in = k.P.xs; a.elem_out = k.P.ys;
    a.inner = k.L.inner; a.lane_in = k.L.lane_in; a.lane_out = k.L.lane_out; a.outer_in = k.L.outer_in; a.outer_out = k.L.outer_out;
    return a;
}

// very short C2C lanes (n = 2..13, 16) that the wavefront kernel did not take: one thread per lane (tiny_kernel.h).
// Column layouts (adjacent lanes contiguous) are coalesced as they are; dense rows are staged through LDS.
static int route_tiny(const Call &k) {
    if (!(k.plan->kind == NDFFT_KIND_C2C && tiny_supported(k.n) && k.P.b.size() <= 2 && tiny_enabled())) return kDeclined;
    const bool stage = k.L.dense;   // 256 lanes x (n | 1) elements of LDS: at most 68 KiB (n = 16, f64)
    set_last_path(stage ? "tiny_row" : k.L.cols ? "tiny_col" : "tiny_strided");
    return launch_tiny(k.plan->dtype, k.n, stage, tiny_args(k, k.P.op == NDFFT_OP_C2C_INV, nullptr), k.stream);
}

// C2C lanes of 14 .. 64 (f64) / 96 (f32) points that factor into two butterflies: one thread per lane, two passes in
// registers (reg_kernel.h), specialised with hiprtc; only worth a compile when there is real work
static int route_reg(const Call &k) {
    const void *mat = k.dt.cfg[CFG_MAIN].wave_tw;
    int n1, n2;
    if (!(k.plan->kind == NDFFT_KIND_C2C && k.n >= 14 && k.n <= regfft_max_n(k.plan->dtype) && mat && k.P.b.size() <= 2 &&
          k.P.nlanes * (int64_t)k.n >= (1 << 16) && tiny_enabled() && !tiny_supported(k.n) && regfft_factor(k.n, &n1, &n2)))
        return kDeclined;
    const bool dense = k.L.dense;
    if (!((dense && k.n <= 63) || (k.L.cols && !dense))) return kDeclined;          // rows beyond 63 points: the general register kernel is faster
    return took(jit_rc(launch_jit_regfft(k.plan->dtype, n1, n2, dense, tiny_args(k, k.P.op == NDFFT_OP_C2C_INV, mat), k.stream)), dense ? "reg_row" : "reg_col");
}

// the real-data transforms on lanes of 12 .. 48 (f64) / 72 (f32) points (from 12 up the butterflies beat the dense matrix of the tiny kernel: n = 16 0.49-0.59 -> see DESIGN 3.0c) whose inner FFT factors into butterflies:
// one thread per lane, everything in registers (reg_kernel.h: RegReal), specialised with hiprtc
static int route_regreal(const Call &k) {
    if (!(k.plan->kind != NDFFT_KIND_C2C && k.n >= 12 && k.n <= regreal_max_n(k.f32() ? 0 : 1) && k.P.b.size() <= 2 &&
          k.P.nlanes * (int64_t)k.n >= (1 << 16) && tiny_enabled()))
        return kDeclined;
    const FftConfig &c = k.plan->cfg[k.slot];
    const DevConfig &d = k.dt.cfg[k.slot];
    int f1, f2;
    if (c.big || !d.wave_tw || !regfft_factor(c.F, &f1, &f2) || !(k.L.dense || k.L.cols)) return kDeclined;   // (c.blue does not matter: primes 17..31 have their own butterfly here)
    RegRealArgs ra;
    ra.t = tiny_args(k, 0, d.wave_tw); ra.aux1 = d.aux1; ra.aux2 = d.aux2;
    return took(jit_rc(launch_jit_regreal(k.plan->dtype, k.gop, k.n, f1, f2, k.L.dense, ra, k.stream)), k.L.dense ? "regreal_row" : "regreal_col");
}

// the real-data transforms on very short lanes (n = 2..16): one thread per lane, the transform as a dense matrix
static int route_tinymat(const Call &k) {
    if (!(k.plan->kind != NDFFT_KIND_C2C && k.n >= 2 && k.n <= 16 && k.P.b.size() <= 2 && tiny_enabled())) return kDeclined;
    const bool r2c = k.plan->kind == NDFFT_KIND_R2C;
    const int q = r2c ? (k.P.op == NDFFT_OP_R2C ? 0 : 1) : k.P.op - NDFFT_OP_DCT1;
    const void *mat = k.dt.cfg[CFG_MAIN].tinymat[q];
    if (!mat) return kDeclined;
    set_last_path(k.L.dense ? "tinymat_row" : k.L.cols ? "tinymat_col" : "tinymat_strided");
    const TinyArgs a = tiny_args(k, 0, mat);
    const int shape = r2c ? q : 2;
    return k.f32() ? launch_tinymat_f32(k.n, shape, k.L.dense, a, k.stream) : launch_tinymat_f64(k.n, shape, k.L.dense, a, k.stream);
}

static Pow2Args c2c_row_args(const Call &k) {
    Pow2Args a;
    a.in = k.in; a.out = k.out; a.nlanes = k.P.nlanes; a.pitch_in = k.L.pitch_in; a.pitch_out = k.L.pitch_out;
    a.inverse = k.P.op == NDFFT_OP_C2C_INV; a.scale = k.P.scale; a.twp = k.dt.cfg[CFG_MAIN].twp;
    return a;
}

// tuned path: contiguous power-of-two C2C lanes at a uniform pitch (the fused filters take the same lanes: compose.hip, filter_fused)
static bool pow2_rows_eligible(const Call &k) { return k.plan->kind == NDFFT_KIND_C2C && k.plan->cfg[CFG_MAIN].pow2 && k.L.rows; }
static int route_pow2_rows(const Call &k) {
    if (!pow2_rows_eligible(k)) return kDeclined;
    Pow2Args a = c2c_row_args(k);
    if (k.L.dense) a.stream_in = c2c_row_load_policy(k.in, k.out, (size_t)k.P.nlanes * k.plan->n * 2 * real_size(k.plan->dtype), &a.keep64, k.plan->dtype == NDFFT_F64);
    set_last_path("pow2_reg");
    return launch_pow2(k.plan->dtype, k.n, a, k.stream);
}

// smooth non-power-of-two C2C lanes: the same register-resident kernel, specialised at first use (jit.hip);
// only worth a compile when there is real work
static int route_jit_rows(const Call &k) {
    if (!(k.plan->kind == NDFFT_KIND_C2C && k.plan->cfg[CFG_MAIN].jit && k.L.rows && k.P.nlanes * (int64_t)k.n >= (1 << 17))) return kDeclined;
    const Pow2Args a = c2c_row_args(k);
    const size_t bytes_c = (size_t)k.P.nlanes * k.plan->n * 2 * real_size(k.plan->dtype);
    const int pol = k.L.dense ? c2c_row_load_policy(k.in, k.out, bytes_c) : -1;
    const int nt = (pol >= 0 ? pol != 0 : stream_loads_for(bytes_c)) ? 3 : 1;
    const int rc = took(jit_rc(launch_jit_c2c(k.plan->dtype, k.plan->cfg[CFG_MAIN].jitcfg, nt, a, k.stream)), "jit_reg");
    if (rc == kDeclined && sw().jit_verbose) fprintf(stderr, "ndfft: jit_reg declined n = %zu\n", k.plan->n);   // declined: the LDS kernel
    return rc;
}

// which kernel of the register-resident real-op engine (pow2_real.h and its hiprtc forms) a call takes, and where
struct Engine {
    bool use_jit, use_rader, use_blue, use_plain, col_alt;
    bool row, col;
};

// long strided lanes on XCD-aware narrow column tiles (one HBM pass)
template <typename T>
static int narrow_tiles(const Call &k) {
    const FftConfig &c = k.plan->cfg[k.slot];
    const DevConfig &d = k.dt.cfg[k.slot];
    RealArgs<T> a{};
    a.in = k.in; a.out = k.out; a.nlanes = k.P.nlanes;
    a.xcd_remap = 1;
    a.n = k.n; a.F = c.F; a.n_in = (int)k.P.xlen; a.n_out = (int)k.P.ylen; a.scale = (T)k.P.scale;
    a.inner = k.L.inner; a.outer_in = k.L.outer_in; a.outer_out = k.L.outer_out;
    a.elem_in = k.P.xs; a.elem_out = k.P.ys;
    a.aux1 = (const cpx<T> *)d.aux1; a.aux2 = (const cpx<T> *)d.aux2; a.twp = (const cpx<T> *)d.twp_narrow;
    const int rc = launch_pow2_real_narrow<T>(k.gop, a, k.stream);
    set_last_path("pow2_col_xcd");
    return rc;
}

// rows or column tiles (strategy ii) on the engine
template <typename T>
static int engine_tiles(const Call &k, const Engine &e) {
    const Problem &P = k.P;
    const FftConfig &c = k.plan->cfg[k.slot];
    const DevConfig &d = k.dt.cfg[k.slot];
    const bool col = e.col, is_c2c = k.plan->kind == NDFFT_KIND_C2C;
    RealArgs<T> a{};
    a.in = k.in; a.out = k.out; a.nlanes = P.nlanes;
    a.pitch_in = k.L.pitch_in; a.pitch_out = k.L.pitch_out;
    a.n = k.n; a.F = c.F; a.n_in = (int)P.xlen; a.n_out = (int)P.ylen; a.scale = (T)P.scale;
    a.inner = col ? k.L.inner : 1; a.outer_in = col ? k.L.outer_in : 0; a.outer_out = col ? k.L.outer_out : 0;
    a.elem_in = P.xs; a.elem_out = P.ys;
    const size_t es_in = (op_in_cplx(P.op) ? 2 : 1) * sizeof(T), es_out = (op_out_cplx(P.op) ? 2 : 1) * sizeof(T);
    a.vec_in = !col && ((uintptr_t)k.in % 16 == 0) && ((size_t)a.pitch_in * es_in) % 16 == 0;
    a.keep_out = P.keep_out; a.stream_in = P.stream_in; a.xcd_chunk = P.no_xcd_map ? 0 : -1;
    a.makhoul = col ? P.makhoul_out : 0;
    // dense rows of the ahead-of-time real-op kernels (BASELINE configs[3]): load policy from the Infinity-Cache model, as for the C2C rows
    // (round 5: also the real-input rows of the Rader kernel)
    if (!col && ((!e.use_jit && !e.use_blue && !e.use_plain) || (e.use_rader && !op_in_cplx(P.op))) && a.pitch_in == P.xlen && a.pitch_out == P.ylen && F_nt_ok(c.F))
        a.stream_in = row_load_policy(k.in, (size_t)P.nlanes * P.xlen * es_in, k.out, (size_t)P.nlanes * P.ylen * es_out) == 1;
    // column tiles of a caller's array (not the stages of col_split / the four-step, which set their own policy): the same model
    if (col && !P.no_xcd_map && !P.stream_in && !P.keep_out)
        a.stream_in = row_load_policy(k.in, (size_t)P.nlanes * P.xlen * es_in, k.out, (size_t)P.nlanes * P.ylen * es_out) == 1;
    a.vec_out = !col && ((uintptr_t)k.out % 16 == 0) && ((size_t)a.pitch_out * es_out) % 16 == 0;
    // R2C rows with dense output lanes: the workgroup stores its lanes as one contiguous chunk (pow2_real.h: chunk_out)
    // Measured (profiles/r03j, 2^24 points f32): n = 96 / 100 48 -> 37 / 32 -> 30 us, powers of two 128..1024 +4 %; n = 500 / 1000 and
    // n >= 2048 lose 2-8 % (fewer, longer lanes per workgroup: the per-lane stores are already long runs), so short lanes only.
    const bool short_lane = c.F <= 64 || (c.F <= 512 && (c.F & (c.F - 1)) == 0);
    a.chunk_out = !col && k.gop == G_R2C_EVEN && short_lane && ((uintptr_t)k.out % 16 == 0) && a.pitch_out == P.ylen;   // (no switch: settled in round 2)
    if (a.chunk_out) a.xcd_chunk = 0;
    a.aux1 = (const cpx<T> *)d.aux1; a.aux2 = (const cpx<T> *)d.aux2; a.twp = (const cpx<T> *)((is_c2c && !e.use_jit && !e.use_blue) ? d.twp_col : d.twp);
    a.chirp = (const cpx<T> *)d.chirp; a.bhat = (const cpx<T> *)d.bhat; a.twp_rev = (const cpx<T> *)d.twp_rev;
    if (e.use_rader) {
        RealArgs<T> r = a;
        r.twp = (const cpx<T> *)d.rader_twp; r.twp_rev = (const cpx<T> *)d.rader_twp2; r.chirp = (const cpx<T> *)d.rader_ctw; r.bhat = (const cpx<T> *)d.rader_bhat;
        r.rader_tab = (const int32_t *)d.rader_tab;
        const int rr = took(jit_rc(launch_jit_rader<T>(k.gop, c.radercfg, col, r, k.stream)), col ? "rader_col" : "rader_reg");
        if (rr != kDeclined) return rr;
    }
    int rc;
    if (e.use_blue) rc = c.bluereg ? launch_jit_blue<T>(k.gop, c.jitcfg, col, a, k.stream) : NDFFT_ERR_UNSUPPORTED;
    else if (e.use_plain) rc = launch_jit_plain<T>(k.gop, c.jitcfg, col, a, k.stream);
    else if (e.use_jit && col && e.col_alt) { a.twp = (const cpx<T> *)d.twp_jcol; rc = launch_jit_real<T>(k.gop, c.jitcfg_col, col, a, k.stream); }
    else if (e.use_jit) rc = launch_jit_real<T>(k.gop, c.jitcfg, col, a, k.stream);
    else rc = launch_pow2_real<T>(k.gop, a, col, k.stream);
    if (e.use_jit || e.use_blue) rc = jit_rc(rc);     // declined: the LDS kernel
    return took(rc, e.use_blue ? (col ? "blue_col" : "blue_reg") : e.use_plain ? (col ? "plain_col" : "plain_real") : e.use_jit ? (col ? "jit_col" : "jit_real") : (col ? "pow2_col" : "pow2_real"));
}

// tuned paths on the register-resident real-op engine (pow2_real.h), power-of-two inner FFT:
//   row: R2C / C2R / DCT on contiguous lanes;  col: the same ops AND C2C on a strided axis whose
//   adjacent lanes are contiguous (strategy ii), through an LDS tile of adjacent lanes
// and, for long strided lanes, the column four-step and the narrow tiles
static int route_real_engine(const Call &k) {
    const Problem &P = k.P;
    const ndfft_plan *plan = k.plan;
    const int gop = k.gop;
    const FftConfig &c = plan->cfg[k.slot];
    const DevConfig &d = k.dt.cfg[k.slot];
    const bool is_c2c = plan->kind == NDFFT_KIND_C2C;
    const bool odd_variant = gop == G_R2C_ODD || gop == G_C2R_ODD || gop == G_DCT2_ODD || gop == G_DCT3_ODD || gop == G_DCT4_ODD;
    Engine e;
    // (2^15 points since round 5: ndfft_r2c axis 0 of the reference's 264 x 264 bench shape is 264 lanes x 132 points -- generic_col 11.6 us, jit_col 6-7 us in a graph;
    //  its code object ships in jit_prebuilt/)
    e.use_jit = c.jit && !c.pow2 && P.nlanes * (int64_t)c.F >= (1 << 15);
    // Bluestein lengths on the register kernel (blue_kernel.h), every op incl. the odd-n variants and row C2C
    // Rader / Good-Thomas (rader_kernel.h) wherever the plan has a recipe -- also for lanes beyond Bluestein's single-launch reach
    // (F > 4096: M' = 2^k >= 2F - 1 no longer fits, Rader's F complex elements of LDS do); Bluestein stays the fallback where it exists
    // (no length rule any more: with the short-lane recipe weights of jit.hip a scan of n = 34..260 has nddct2 on Rader at a median 1.59x over Bluestein with two lengths
    //  7 % slower, C2C at 1.7x with none, profiles/r04/r04zd_rader_short_real.txt)
    e.use_rader = c.rader && P.nlanes * (int64_t)c.F >= (1 << 16) && blue_enabled();
    e.use_blue = e.use_rader || (c.bluereg && ((P.nlanes * (int64_t)c.M >= (1 << 16) && blue_enabled()) || c.blue_reg_only));
    e.use_plain = odd_variant && e.use_jit && !e.use_blue && plain_enabled();         // odd-n real ops with a smooth inner FFT: plain_kernel.h
    const bool have_tw = e.use_jit || e.use_blue || (is_c2c ? !c.twp_col.re.empty() : c.pow2);
    // column tiles of a C2C plan may have their own recipe (FftConfig::jit_col_alt)
    e.col_alt = e.use_jit && !e.use_blue && !e.use_plain && is_c2c && c.jit_col_alt;
    const JitCfg &jcol = e.col_alt ? c.jitcfg_col : c.jitcfg;
    e.row = (!is_c2c || e.use_blue) && k.L.rows;
    e.col = false;
    bool narrow = false;
    const int col_kind = is_c2c ? 0 : (P.op == NDFFT_OP_R2C ? 1 : (P.op == NDFFT_OP_C2R ? 2 : 3));   // which sides of a column tile are real lanes (kernels_pow2_real.hip: ColGeom)
    if (!e.row && (!odd_variant || e.use_blue || e.use_plain) && P.xlen > 1 && k.L.cols && P.b.size() <= 2) {
        if (have_tw && k.L.inner >= 8) {
            const int lanes = (e.use_jit || e.use_blue) ? std::max((e.use_jit || c.bluereg) ? jit_col_lanes(plan->dtype, e.use_blue ? c.jitcfg : jcol, is_c2c && e.use_jit && !e.use_blue) : 0, e.use_rader ? rader_col_lanes(plan->dtype, c.radercfg) : 0)
                                                    : k.f32() ? pow2_real_col_lanes<float>(c.F, col_kind) : pow2_real_col_lanes<double>(c.F, col_kind);
            e.col = lanes > 0;
        }
        // long lanes: XCD-aware narrow tiles (one HBM pass) instead of the three-pass transpose route (no switch: the transpose route is the fallback)
        // (not for the DCTs since round 3: transpose -> row kernel -> transpose measured faster -- nddct2 axis 0 of 4096 x 4096 / 8192 x 2048 f32 166 / 172 -> 100 / 103 us,
        //  f64 174 / 283 -> 164 / 190 us, profiles/r06/r06z_*; C2R f64 n = 4096 stays: 126 vs 174 us)
        if (!e.col && (col_kind != 3 || narrow_dct_enabled()) && !c.twp_narrow.re.empty() && k.L.inner >= 64) {
            const int lanes = k.f32() ? pow2_real_narrow_lanes<float>(c.F) : pow2_real_narrow_lanes<double>(c.F);
            narrow = lanes > 0;
        }
    }
    // long strided power-of-two lanes on a dense C-layout block: column four-step (two wide-tile passes)
    if (c.cs && k.slot == CFG_MAIN && colsplit_enabled() && !e.row && k.L.cols && P.b.size() <= 2 && P.xs == k.L.inner && P.ys == k.L.inner && k.L.inner >= 16 &&
        (((P.op == NDFFT_OP_C2C_FWD || P.op == NDFFT_OP_C2C_INV) && (c.cs_ops & 1)) || (P.op == NDFFT_OP_R2C && (c.cs_ops & 2)) || (P.op == NDFFT_OP_C2R && (c.cs_ops & 4))))
        return k.f32() ? col_split<float>(P, k.in, k.out, c, d, k.stream) : col_split<double>(P, k.in, k.out, c, d, k.stream);
    if (narrow) return k.f32() ? narrow_tiles<float>(k) : narrow_tiles<double>(k);
    if (have_tw && (!odd_variant || e.use_blue || e.use_plain) && (e.row || e.col)) return k.f32() ? engine_tiles<float>(k, e) : engine_tiles<double>(k, e);
    return kDeclined;
}

// long lanes: four-step on the row kernels (contiguous lanes) -- strided ones reach here via the transpose route
static int route_long(const Call &k) {
    if (k.plan->cfg[k.slot].unsupported)
        return fail(NDFFT_ERR_UNSUPPORTED, "lane length has a prime factor too large for the single-launch Bluestein and no usable "
                                           "four-step split (DESIGN.md section 9)");
    if (!(k.plan->cfg[k.slot].big && k.L.rows)) return kDeclined;
    return k.f32() ? dispatch_big<float>(k.P, k.in, k.out, k.dt, k.stream) : dispatch_big<double>(k.P, k.in, k.out, k.dt, k.stream);
}

// a route that ran another dispatch() inside: its path is "<prefix><inner path>"
int prefixed(const char *prefix, int rc) {
    if (rc == NDFFT_OK) {
        static thread_local std::string path;
        path = std::string(prefix) + last_path();
        set_last_path(path.c_str());
    }
    return rc;
}

// strided axis of a C-layout array whose lanes are too long for a useful LDS tile of adjacent
// lanes (< 128 B contiguous per tile row): go through the batched transpose
static int route_transposed(const Call &k) {
    const Problem &P = k.P;
    if (!(P.xs != 1 && P.ys != 1 && P.xlen > 1 && k.L.cols && P.b.size() <= 2)) return kDeclined;
    const int64_t inner = k.L.inner;
    const int64_t outer = P.b.size() == 2 ? P.b[0].shape : 1;
    const size_t r = real_size(k.plan->dtype);
    const size_t ein = op_in_cplx(P.op) ? 2 * r : r, eout = op_out_cplx(P.op) ? 2 * r : r;
    const bool c_layout = P.xs == inner && P.ys == inner && (P.b.size() == 1 || (P.b[0].sin == P.xlen * inner && P.b[0].sout == P.ylen * inner));
    // LDS bytes one lane needs in the generic kernel (two padded complex buffers)
    const FftConfig &c = k.plan->cfg[k.slot];
    const size_t per_lane = 2 * (size_t)generic_z_len(std::max(c.blue ? c.M : c.F, 1)) * 2 * r;
    const size_t fit = c.big ? 0 : (160 * 1024 - 2048) / std::max<size_t>(per_lane, 1);
    const size_t row_bytes = std::min<size_t>(fit, (size_t)inner) * std::min(ein, eout);
    if (!(c_layout && row_bytes < 128 && (inner >= 16 || c.big))) return kDeclined;
    return prefixed("transpose+", dispatch_transposed(P, k.in, k.out, k.stream, outer, inner, ein, eout));
}

// long lanes in an arbitrary strided layout: pack -> row path on dense lanes -> unpack
static int route_packed(const Call &k) {
    const Problem &P = k.P;
    if (!k.plan->cfg[k.slot].big) return kDeclined;
    const size_t r = real_size(k.plan->dtype);
    const size_t ein = op_in_cplx(P.op) ? 2 * r : r, eout = op_out_cplx(P.op) ? 2 * r : r;
    void *s1, *s2;
    int rc;
    if ((rc = get_scratch(0, k.stream, (size_t)(P.nlanes * P.xlen) * ein, &s1))) return rc;
    if ((rc = get_scratch(1, k.stream, (size_t)(P.nlanes * P.ylen) * eout, &s2))) return rc;
    LaneGeom gi, go;
    gi.axis_stride = P.xs; go.axis_stride = P.ys; gi.nb = go.nb = (int32_t)P.b.size(); gi.pad_ = go.pad_ = 0;
    for (size_t i = 0; i < P.b.size(); ++i) { gi.bshape[i] = go.bshape[i] = P.b[i].shape; gi.bstride[i] = P.b[i].sin; go.bstride[i] = P.b[i].sout; }
    if ((rc = launch_pack_lanes(k.in, s1, gi, P.nlanes, P.xlen, P.xlen, (int)ein, 0, k.stream))) return rc;
    Problem Q = P;
    Q.xs = Q.ys = 1; Q.b.clear(); Q.b.push_back({P.nlanes, P.xlen, P.ylen});
    if ((rc = dispatch(Q, s1, s2, k.stream))) return rc;
    return prefixed("pack+", launch_pack_lanes(k.out, s2, go, P.nlanes, P.ylen, P.ylen, (int)eout, 1, k.stream));
}

// the routes in order of preference; the generic LDS kernel takes whatever none of them does
int dispatch(const Problem &P, const void *d_in, void *d_out, hipStream_t stream) {
    const DevTables *dt;
    int rc = get_dev_tables(P.plan, &dt);
    if (rc) return rc;
    const Call k(P, d_in, d_out, stream, *dt);
    for (int (*route)(const Call &) : {route_wave, route_tiny, route_reg, route_regreal, route_tinymat, route_pow2_rows, route_jit_rows,
                                       route_real_engine, route_long, route_transposed, route_packed})
        if ((rc = route(k)) != kDeclined) return rc;
    return k.f32() ? dispatch_generic<float>(P, d_in, d_out, *dt, stream) : dispatch_generic<double>(P, d_in, d_out, *dt, stream);
}

}  // namespace ndfft

using namespace ndfft;

extern "C" {

int ndfft_exec_device(const ndfft_plan *plan, int op, const void *d_in, void *d_out, int ndim,
                      const int64_t *shape_in, const int64_t *stride_in, const int64_t *shape_out,
                      const int64_t *stride_out, int axis, int norm, double scale, void *stream) {
    clear_err();
    reset_last_policy();
    Problem P;
    bool nothing;
    int rc = prepare(plan, op, ndim, shape_in, stride_in, shape_out, stride_out, axis, norm, scale, P, nothing);
    if (rc || nothing) return rc;
    if (!d_in || !d_out) return fail(NDFFT_ERR_INVALID_ARG, "null array pointer");
    const size_t r = real_size(plan->dtype);
    return dispatch_peeled(P, (const char *)d_in, (char *)d_out, op_in_cplx(op) ? 2 * r : r, op_out_cplx(op) ? 2 * r : r,
                           (hipStream_t)stream);
}

int ndfft_last_input_policy(void) { return g_last_policy; }
int ndfft_last_input_keep(void) { return g_last_keep; }
int ndfft_set_keep_budget(int mib) {
    clear_err();
    if (mib > (1 << 20)) return fail(NDFFT_ERR_INVALID_ARG, "keep budget beyond 2^20 MiB");
    g_keep_budget_mb = mib < 0 ? -1 : mib;
    return NDFFT_OK;
}
int ndfft_force_input_keep(int keep64) {
    clear_err();
    if (keep64 > 64) return fail(NDFFT_ERR_INVALID_ARG, "kept share beyond 64");
    g_keep_force = keep64 < 0 ? -1 : keep64;
    return NDFFT_OK;
}

int ndfft_set_input_hint(int hint) {
    clear_err();
    if (hint < NDFFT_INPUT_AUTO || hint > NDFFT_INPUT_COLD) return fail(NDFFT_ERR_INVALID_ARG, "bad input hint");
    g_input_hint = hint;
    return NDFFT_OK;
}

int ndfft_release_workspace(void) {
    clear_err();
    g_tws.release_all();   // every device this thread has used; each synchronised under its own hipSetDevice
    shard_release_all();   // and the chunk buffers of the multi-device workers (up to 4 x 64 MiB per worker)
    return NDFFT_OK;
}

}  // extern "C"

// host.hip is a unit of its own (-DNDFFT_HOST_UNIT, set by every build list that names it).  A list of objects written before it
// existed does not name it and would link a library without ndfft_exec: such a build gets the host-array call through this unit.
#ifndef NDFFT_HOST_UNIT
#include "host.hip"
#endif
// ... and so is compose.hip (-DNDFFT_COMPOSE_UNIT): an older list gets dispatch_peeled and the weighted and filter calls through this unit
#ifndef NDFFT_COMPOSE_UNIT
#include "compose.hip"
#endif
