// compose.hip -- the calls that are made of dispatch() (exec.hip) and something around it: the host-side peel of surplus batch dims, Normalization::Weights
// (ndfft_exec_weighted_device: a diagonal pass in front of or behind the transform) and the spectral filters (ndfft_exec_filter_device,
// ndfft_exec_dct_filter_device: forward transform, weights, inverse transform -- fused into one kernel where kernels_filter.hip has one, composed otherwise).
// What it takes from exec.hip is declared in exec_internal.h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "exec_internal.h"
#include "../../include/ndfft_mi355x_ext.h"

namespace ndfft {

// more than kMaxBatchDims un-mergeable batch dims: the slowest ones are peeled on the host; one(Q, in, out) runs every piece of at most kMaxBatchDims
template <class F> static int peeled(Problem &P, const char *in, char *out, size_t ein, size_t eout, F &&one) {
    if (P.b.size() <= (size_t)kMaxBatchDims) return one(P, in, out);
    const BatchDim outer = P.b.front();
    Problem Q = P;
    Q.b.erase(Q.b.begin());
    Q.nlanes = P.nlanes / outer.shape;
    for (int64_t i = 0; i < outer.shape; ++i) {
        int rc = peeled(Q, in + i * outer.sin * (int64_t)ein, out + i * outer.sout * (int64_t)eout, ein, eout, one);
        if (rc) return rc;
    }
    return NDFFT_OK;
}
int dispatch_peeled(Problem &P, const char *d_in, char *d_out, size_t ein, size_t eout, hipStream_t stream) {
    return peeled(P, d_in, d_out, ein, eout, [&](const Problem &Q, const char *in, char *out) { return dispatch(Q, in, out, stream); });
}

static void lane_geoms(const Problem &P, LaneGeom &gi, LaneGeom &go) {
    gi.axis_stride = P.xs; go.axis_stride = P.ys; gi.nb = go.nb = (int32_t)P.b.size(); gi.pad_ = go.pad_ = 0;
    for (size_t i = 0; i < P.b.size(); ++i) { gi.bshape[i] = go.bshape[i] = P.b[i].shape; gi.bstride[i] = P.b[i].sin; go.bstride[i] = P.b[i].sout; }
}
// a route followed by the weight pass: its path is "<route>+weights"
static int suffixed(int rc, const char *suffix) {
    if (rc == NDFFT_OK) {
        static thread_local std::string path;
        path = std::string(last_path()) + suffix;
        set_last_path(path.c_str());
    }
    return rc;
}
// The dims of the INPUT view, fastest first by |stride|: order[k] indexes P.b, and nd - 1 (the returned count less one) names the axis.  A dense image that gives
// its dims positive strides in this order keeps the input's own dimension order, so that a transform on the image takes the route it would take on the caller's array.
static int dense_order(const Problem &P, int (&order)[kMaxBatchDims + 1]) {
    const int nd = (int)P.b.size() + 1;
    auto stride_of = [&](int i) { return i == nd - 1 ? P.xs : P.b[i].sin; };
    for (int i = 0; i < nd; ++i) order[i] = i;
    std::stable_sort(order, order + nd, [&](int a, int b) {
        const int64_t sa = std::llabs(stride_of(a)), sb = std::llabs(stride_of(b));
        return sa != sb ? sa < sb : a > b;           // equal strides (extent-1 lanes): the later dim is the faster one, as in C order
    });
    return nd;
}

// ---------------------------------------------------------------------------------------------
// Normalization::Weights (ndfft_exec_weighted_device): the diagonal pass of weights_kernel.h around dispatch(), at the reference's
// application points.  The transform itself runs with scale 1 on the route it would take anyway.
// ---------------------------------------------------------------------------------------------
// one problem of <= kMaxBatchDims batch dims
static int weighted(const Problem &P, const char *d_in, char *d_out, const void *d_w, hipStream_t stream) {
    const int dtype = P.plan->dtype;
    int rc;
    LaneGeom gi, go;
    if (P.op == NDFFT_OP_C2C_INV) {
        // after, on the output lane (lib.rs:326-330): in place on the output view, the final result -> streaming stores like the transform kernels' own
        if ((rc = dispatch(P, d_in, d_out, stream))) return rc;
        lane_geoms(P, gi, go);
        return suffixed(launch_weights(d_out, d_out, d_w, go, go, P.ylen, dtype, 1, 1, stream), "+weights");
    }
    // before, on the input lane (lib.rs:511-515, 692-696): caller's input -> a dense image in the input's own dimension order (dense_order); a broadcast BATCH dim
    // keeps stride 0 and is not materialised
    const int cplx = op_in_cplx(P.op) ? 1 : 0;
    const size_t ein = real_size(dtype) * (cplx ? 2 : 1);
    Problem Q = P;
    int order[kMaxBatchDims + 1];
    const int nd = dense_order(P, order);
    int64_t run = 1;
    for (int k = 0; k < nd; ++k) {
        const int i = order[k];
        // (only a BATCH dim may stay broadcast: a diagonal does not commute with broadcasting along the lane, x * w[j] differs from j to j, so the axis is always materialised)
        if (i == nd - 1) { Q.xs = run; run *= P.xlen; }
        else if (P.b[i].sin == 0) Q.b[i].sin = 0;
        else { Q.b[i].sin = run; run *= P.b[i].shape; }
    }
    void *S;
    if ((rc = get_scratch(8, stream, (size_t)run * ein, &S))) return rc;
    DeviceWs *ws;
    if ((rc = current_ws(&ws))) return rc;
    lane_geoms(P, gi, go);
    LaneGeom gq, unused;
    lane_geoms(Q, gq, unused);
    // the image is read again at once by the transform: plain, cache-allocating stores
    if ((rc = launch_weights(d_in, S, d_w, gi, gq, P.xlen, dtype, cplx, 0, stream))) return rc;
    // Speed only: what the row kernels' load policy should expect of the image.  Noted BEFORE dispatch() on purpose, so that a route with a load policy sees the image as
    // just written (small: resident, plain loads; above 64 MiB: streaming loads); that route's own row_load_policy then notes the read.  Routes without a policy leave the
    // read un-noted.  Neither choice has been measured against the alternative.
    ws->mall.note_write(S, (size_t)run * ein);
    return prefixed("weights+", dispatch(Q, S, d_out, stream));
}

// ---------------------------------------------------------------------------------------------
// The filters: out = s INV(w (.) FWD(in)) along the axis.  P is the FORWARD problem from the caller's input geometry to the caller's OUTPUT geometry (sin / xs: input
// strides, sout / ys: output strides; for an R2C plan P.ylen is the half spectrum's length, the output lane has P.xlen reals).  One record per plan kind says what
// differs between the three.
// ---------------------------------------------------------------------------------------------
struct FilterMode {
    int mode;                          // FILTER_* of the fused kernel (engine.h)
    int fwd, inv;                      // the two ops
    int array_reals, image_reals;      // reals per element of the caller's arrays, of the spectrum image of the composed route
    int weights_cplx;                  // the diagonal pass on the image: 1 = the complex product, 0 = real weights on real elements (as Normalization::Weights uses it for the DCT ops)
    const char *lane_word;             // what the n_weights message calls the weighted lane
    double (*default_scale)(double n); // NDFFT_NORM_DEFAULT
    const char *path;                  // the fused route's
    // fused route: can the kernel address these lanes (rows at the REAL pitches pin / pout)?  Turns the pitches into the kernel's unit
    bool (*lanes)(int64_t &pin, int64_t &pout, const void *in, const void *out, size_t r);
    int (*tables)(const ndfft_plan *plan, FilterArgs &f);     // what the kernel reads beside the plan's own twp, which filter_fused has set
};
static bool any_lanes(int64_t &, int64_t &, const void *, const void *, size_t) { return true; }
static const FilterMode kFilterC2c = {
    FILTER_C2C, NDFFT_OP_C2C_FWD, NDFFT_OP_C2C_INV, 2, 2, 1, "spectrum", [](double n) { return 1.0 / n; }, "filter_pow2",
    // pitches in complex elements, as Problem has them
    any_lanes,
    [](const ndfft_plan *plan, FilterArgs &f) { return get_filter_twiddles(plan, &f.twp_rev); }};
static const FilterMode kFilterR2c = {
    FILTER_R2C, NDFFT_OP_R2C, NDFFT_OP_C2R, 1, 2, 1, "spectrum", [](double n) { return 1.0 / n; }, "filter_r2c_pow2",
    // the lane is read as n / 2 complex points: every lane base must be a whole complex element -- bases multiples of 2 sizeof(T), even pitches
    [](int64_t &pin, int64_t &pout, const void *in, const void *out, size_t r) {
        if (!(pin % 2 == 0 && pout % 2 == 0 && (uintptr_t)in % (2 * r) == 0 && (uintptr_t)out % (2 * r) == 0)) return false;
        pin /= 2; pout /= 2;
        return true;
    },
    [](const ndfft_plan *plan, FilterArgs &f) { return get_filter_r2c_tables(plan, &f.a.twp, &f.twp_rev, &f.wn); }};
static const FilterMode kFilterDct = {
    // nddct2 and nddct3 each pre-scale their input by 2 under Default (lib.rs:700-722, 736-741): both factors are exact, so the pair's is 4
    FILTER_DCT, NDFFT_OP_DCT2, NDFFT_OP_DCT3, 1, 1, 0, "coefficient", [](double) { return 4.0; }, "filter_dct_pow2",
    // NO alignment condition: the kernel reads and writes the lane as reals
    any_lanes,
    [](const ndfft_plan *plan, FilterArgs &f) { return get_filter_r2c_tables(plan, &f.a.twp, &f.twp_rev, &f.wn, &f.c); }};

// fused, C2C along a strided axis: the fastest batch dim has unit stride in both views (axis 0 of a 2-D C-layout array, the middle axis of a 3-D one, windows of
// either), at most two batch dims, at least 8 adjacent lanes (the column engine's own rule, exec.hip: route_real_engine) and a length from 128 that has a column
// instance -- one launch of column tiles, path filter_col_pow2.  Everything else stays composed.
static int filter_fused_col(const FilterMode &m, const Problem &P, const Layout &L, const DevTables *dt, const char *d_in, char *d_out, const void *d_w, hipStream_t stream) {
    const int dtype = P.plan->dtype, n = (int)P.plan->n;
    if (!(L.cols && P.b.size() <= 2 && L.inner >= 8 && n >= 128 && filter_col_supported(dtype, n))) return kDeclined;
    FilterArgs f;
    f.a.in = d_in; f.a.out = d_out; f.a.nlanes = P.nlanes; f.a.pitch_in = f.a.pitch_out = 0;
    f.a.inverse = 0; f.a.scale = P.scale; f.a.twp = dt->cfg[CFG_MAIN].twp;
    f.w = d_w;
    f.inner = L.inner; f.outer_in = L.outer_in; f.outer_out = L.outer_out; f.elem_in = P.xs; f.elem_out = P.ys;
    int rc = m.tables(P.plan, f);
    if (rc) return rc;
    // a dense C-layout block: the whole array is read once and written once, as the row kernel's dense lanes are
    const bool dense = P.xs == L.inner && P.ys == L.inner && (P.b.size() == 1 || (L.outer_in == n * L.inner && L.outer_out == n * L.inner));
    if (dense) f.a.stream_in = c2c_row_load_policy(d_in, d_out, (size_t)P.nlanes * P.plan->n * m.array_reals * real_size(dtype));
    set_last_path("filter_col_pow2");
    return launch_filter_col(dtype, n, f, stream);
}

// fused: lanes of n = 64 .. 4096 complex points (128 .. 8192 reals) at unit stride along the axis and a uniform pitch, on which dispatch() would run pow2_reg in both
// directions -- one launch, no scratch.  The first call of a plan builds and uploads the tables it lacks (get_filter_twiddles: none for a palindromic radix list;
// get_filter_r2c_tables); later calls allocate nothing.
static int filter_fused(const FilterMode &m, const Problem &P, const char *d_in, char *d_out, const void *d_w, hipStream_t stream) {
    const DevTables *dt;
    int rc = get_dev_tables(P.plan, &dt);
    if (rc) return rc;
    const int dtype = P.plan->dtype, n = (int)P.plan->n;
    const Layout L(P);
    if (!L.rows) return m.mode == FILTER_C2C ? filter_fused_col(m, P, L, dt, d_in, d_out, d_w, stream) : kDeclined;
    if (!filter_supported(m.mode, dtype, n)) return kDeclined;
    // in reals or complex elements as the arrays have them (Layout's pitch_out is the half spectrum's for an R2C plan without a batch dim)
    int64_t pin = P.b.empty() ? n : P.b[0].sin, pout = P.b.empty() ? n : P.b[0].sout;
    const bool dense = pin == n && pout == n;
    if (!m.lanes(pin, pout, d_in, d_out, real_size(dtype))) return kDeclined;
    FilterArgs f;
    f.a.in = d_in; f.a.out = d_out; f.a.nlanes = P.nlanes; f.a.pitch_in = pin; f.a.pitch_out = pout;
    f.a.inverse = 0; f.a.scale = P.scale; f.a.twp = dt->cfg[CFG_MAIN].twp;
    f.w = d_w;
    if ((rc = m.tables(P.plan, f))) return rc;
    if (dense) f.a.stream_in = c2c_row_load_policy(d_in, d_out, (size_t)P.nlanes * P.plan->n * m.array_reals * real_size(dtype));
    set_last_path(m.path);
    return launch_filter(m.mode, dtype, n, f, stream);
}
// adjacent batch dims that are contiguous in both views become one (as prepare() does)
static void remerge(Problem &Q) {
    std::vector<BatchDim> b;
    for (const BatchDim &d : Q.b) {
        if (!b.empty() && b.back().sin == d.shape * d.sin && b.back().sout == d.shape * d.sout) { b.back().shape *= d.shape; b.back().sin = d.sin; b.back().sout = d.sout; continue; }
        b.push_back(d);
    }
    Q.b.swap(b);
}
// composed, one problem of <= kMaxBatchDims batch dims: forward dispatch() into a dense spectrum image S (in the input's own dimension order, as weighted() builds its
// image, but with every dim materialised: the spectrum of a broadcast lane is written once per index), the diagonal pass in place on S (cache-allocating stores: the
// inverse reads it at once), inverse dispatch() from S into the caller's output.  S is scratch slot 8, which no route's own scratch aliases.  Safe in place: the whole
// input is in S before the inverse writes.
static int filter_composed(const FilterMode &m, const Problem &P, const char *d_in, char *d_out, const void *d_w, hipStream_t stream) {
    const int dtype = P.plan->dtype;
    const size_t ec = m.image_reals * real_size(dtype);
    int order[kMaxBatchDims + 1];
    const int nd = dense_order(P, order);
    Problem F = P, I = P;                          // F: caller's input -> S;  I: S -> caller's output
    F.op = m.fwd; F.scale = 1.0;
    I.op = m.inv; I.xlen = P.ylen; I.ylen = P.xlen;   // (I.scale: the call's)
    int64_t run = 1;
    for (int k = 0; k < nd; ++k) {
        const int i = order[k];
        if (i == nd - 1) { F.ys = I.xs = run; run *= P.ylen; }
        else { F.b[i].sout = I.b[i].sin = run; run *= P.b[i].shape; }
    }
    remerge(F); remerge(I);
    void *S;
    int rc;
    if ((rc = get_scratch(8, stream, (size_t)run * ec, &S))) return rc;
    DeviceWs *ws;
    if ((rc = current_ws(&ws))) return rc;
    if ((rc = dispatch(F, d_in, S, stream))) return rc;
    static thread_local std::string path;
    const std::string fwd = last_path();
    LaneGeom gs, unused;
    lane_geoms(I, gs, unused);
    if ((rc = launch_weights(S, S, d_w, gs, gs, P.ylen, dtype, m.weights_cplx, 0, stream))) return rc;
    ws->mall.note_write(S, (size_t)run * ec);      // (speed only, as in weighted(): what a row kernel's load policy should expect of the image)
    if ((rc = dispatch(I, S, d_out, stream))) return rc;
    path = fwd + "+weights+" + last_path();
    set_last_path(path.c_str());
    return NDFFT_OK;
}

// The body of both filter entry points.  The checks are those of ndfft_exec_device for the mode's forward op, in its order: a plan of another kind fails inside
// prepare ("op does not belong to this plan's handler kind"), a call with nothing to do returns before the pointers and the weights are looked at.
static int exec_filter(const FilterMode &m, const ndfft_plan *plan, const void *d_in, void *d_out, int ndim, const int64_t *shape, const int64_t *stride_in,
                       const int64_t *stride_out, int axis, const void *d_weights, size_t n_weights, int norm, double scale, int flags, void *stream) {
    clear_err();
    reset_last_policy();
    // the forward op of an R2C plan maps the caller's real lane to a half spectrum, so its output extent along the axis is n / 2 + 1 whatever the caller's is
    int64_t shape_mid[NDFFT_MAX_DIMS];
    const int64_t *shape_out = shape;
    if (m.fwd == NDFFT_OP_R2C && shape && ndim > 0 && ndim <= NDFFT_MAX_DIMS && axis >= 0 && axis < ndim) {
        for (int d = 0; d < ndim; ++d) shape_mid[d] = shape[d];
        shape_mid[axis] = (int64_t)plan->n / 2 + 1;
        shape_out = shape_mid;
    }
    Problem P;
    bool nothing;
    int rc = prepare(plan, m.fwd, ndim, shape, stride_in, shape_out, stride_out, axis, norm, scale, P, nothing);
    if (rc || nothing) return rc;
    if (!d_in || !d_out) return fail(NDFFT_ERR_INVALID_ARG, "null array pointer");
    if (!d_weights) return fail(NDFFT_ERR_INVALID_ARG, "null weights pointer");
    if ((int64_t)n_weights != P.ylen) {
        char msg[128];
        snprintf(msg, sizeof msg, "weights: got %zu expected %lld (the length of the %s lane)", n_weights, (long long)P.ylen, m.lane_word);
        return fail(NDFFT_ERR_INVALID_ARG, msg);
    }
    if (flags & ~NDFFT_FILTER_NO_FUSE) return fail(NDFFT_ERR_INVALID_ARG, "unknown filter flag");
    P.scale = norm == NDFFT_NORM_NONE ? 1.0 : norm == NDFFT_NORM_DEFAULT ? m.default_scale((double)plan->n) : scale;   // of the fused kernel, of the composed route's inverse
    const bool fuse = !(flags & NDFFT_FILTER_NO_FUSE);
    const hipStream_t s = (hipStream_t)stream;
    const size_t esz = m.array_reals * real_size(plan->dtype);
    return peeled(P, (const char *)d_in, (char *)d_out, esz, esz, [&](const Problem &Q, const char *in, char *out) {
        const int frc = fuse ? filter_fused(m, Q, in, out, d_weights, s) : kDeclined;
        return frc != kDeclined ? frc : filter_composed(m, Q, in, out, d_weights, s);
    });
}

}  // namespace ndfft

using namespace ndfft;

extern "C" {

int ndfft_exec_weighted_device(const ndfft_plan *plan, int op, const void *d_in, void *d_out, int ndim,
                               const int64_t *shape_in, const int64_t *stride_in, const int64_t *shape_out,
                               const int64_t *stride_out, int axis, const void *d_weights, size_t n_weights, void *stream) {
    clear_err();
    reset_last_policy();
    Problem P;
    bool nothing;
    int rc = prepare(plan, op, ndim, shape_in, stride_in, shape_out, stride_out, axis, NDFFT_NORM_NONE, 0.0, P, nothing);
    if (rc || nothing) return rc;
    if (!d_in || !d_out) return fail(NDFFT_ERR_INVALID_ARG, "null array pointer");
    const size_t r = real_size(plan->dtype);
    const size_t ein = op_in_cplx(op) ? 2 * r : r, eout = op_out_cplx(op) ? 2 * r : r;
    const hipStream_t s = (hipStream_t)stream;
    if (op == NDFFT_OP_C2C_FWD || op == NDFFT_OP_R2C)   // the forward lane methods never look at the normalisation (lib.rs:313-318, 497-503)
        return dispatch_peeled(P, (const char *)d_in, (char *)d_out, ein, eout, s);
    if (!d_weights) return fail(NDFFT_ERR_INVALID_ARG, "null weights pointer");
    const int64_t want = op == NDFFT_OP_C2C_INV ? P.ylen : P.xlen;
    if ((int64_t)n_weights != want) {
        char m[128];
        snprintf(m, sizeof m, "weights: got %zu expected %lld (the length of the weighted lane)", n_weights, (long long)want);
        return fail(NDFFT_ERR_INVALID_ARG, m);
    }
    return peeled(P, (const char *)d_in, (char *)d_out, ein, eout,
                  [&](const Problem &Q, const char *in, char *out) { return weighted(Q, in, out, d_weights, s); });
}

// (a DCT plan has no forward op here, a C2C or an R2C plan none in the DCT call: prepare refuses them)
int ndfft_exec_filter_device(const ndfft_plan *plan, const void *d_in, void *d_out, int ndim, const int64_t *shape, const int64_t *stride_in,
                             const int64_t *stride_out, int axis, const void *d_weights, size_t n_weights, int norm, double scale, int flags, void *stream) {
    const FilterMode &m = plan && plan->kind == NDFFT_KIND_R2C ? kFilterR2c : kFilterC2c;
    return exec_filter(m, plan, d_in, d_out, ndim, shape, stride_in, stride_out, axis, d_weights, n_weights, norm, scale, flags, stream);
}
int ndfft_exec_dct_filter_device(const ndfft_plan *plan, const void *d_in, void *d_out, int ndim, const int64_t *shape, const int64_t *stride_in,
                                 const int64_t *stride_out, int axis, const void *d_weights, size_t n_weights, int norm, double scale, int flags, void *stream) {
    return exec_filter(kFilterDct, plan, d_in, d_out, ndim, shape, stride_in, stride_out, axis, d_weights, n_weights, norm, scale, flags, stream);
}

}  // extern "C"
