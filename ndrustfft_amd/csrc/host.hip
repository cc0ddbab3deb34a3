// host.hip -- ndfft_exec: one nd* call on the caller's own host arrays, the only call the reference's signature can make (src/lib.rs:105-115).
// The arrays are staged through HBM by one of four strategies, tried in order (the routes at the end of this file): mapped bounce buffers
// for small calls, a chunk pipeline straight on pinned / registered arrays, the same pipeline through pinned bounce buffers for pageable
// ones, plain synchronous copies.  Validation and kernel choice are exec.hip's (prepare, dispatch), reached through compose.hip's dispatch_peeled (exec_internal.h);
// docs/host_path.md has the map.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#if defined(__x86_64__) && !defined(NDFFT_NO_NT_COPY)
#include <immintrin.h>   // host-side streaming copy of the bounce pipeline (bulk_copy)
#endif

#include "exec_internal.h"

namespace ndfft {

// element range [lo, hi] (inclusive, relative to element 0) touched by a view
void view_range(int ndim, const int64_t *shape, const int64_t *stride, int64_t &lo, int64_t &hi, int64_t &count) {
    lo = hi = 0; count = 1;
    for (int d = 0; d < ndim; ++d) {
        count *= shape[d];
        if (shape[d] <= 0) continue;
        const int64_t ext = (shape[d] - 1) * stride[d];
        if (ext < 0) lo += ext; else hi += ext;
    }
}

// Copies exactly the elements of an n-d view between two byte images of the same address range (`dst` and `src`
// both point at the image of element 0).  Used for output views with holes: the device result comes back as an
// image of the view's whole span, and only the elements the view OWNS may be written to the caller's memory --
// Rust's `&mut ArrayViewMut` guarantees exclusivity of those elements only (two threads may hold interleaved
// views of one allocation, e.g. even / odd columns from multi_slice_mut).
static void copy_view_elements(char *dst, const char *src, int ndim, const int64_t *shape, const int64_t *stride, size_t esz) {
    struct D { int64_t n, s; };
    std::vector<D> d;
    for (int k = 0; k < ndim; ++k) {
        if (shape[k] == 0) return;
        if (shape[k] > 1 && stride[k] != 0) d.push_back({shape[k], stride[k]});
    }
    std::sort(d.begin(), d.end(), [](const D &a, const D &b) { return std::llabs(a.s) < std::llabs(b.s); });
    // innermost contiguous run (|stride| == 1), merged with outer dims that continue it
    int64_t run = 1, run_off = 0;   // run_off: offset of the run's lowest element relative to the index-0 element
    size_t first = 0;
    if (!d.empty() && std::llabs(d[0].s) == 1) {
        run = d[0].n; run_off = d[0].s < 0 ? -(d[0].n - 1) : 0; first = 1;
        while (first < d.size() && d[first].s == run && run_off == 0) { run *= d[first].n; ++first; }
    }
    std::vector<D> o(d.begin() + first, d.end());
    std::vector<int64_t> idx(o.size(), 0);
    int64_t off = 0;
    for (;;) {
        memcpy(dst + (off + run_off) * (int64_t)esz, src + (off + run_off) * (int64_t)esz, (size_t)run * esz);
        size_t k = 0;
        for (; k < o.size(); ++k) {
            off += o[k].s;
            if (++idx[k] < o[k].n) break;
            off -= o[k].s * o[k].n; idx[k] = 0;
        }
        if (k == o.size()) break;
    }
}

}  // namespace ndfft

using namespace ndfft;

namespace {
// ---- pinned host arrays: H2D || kernel || D2H over row chunks --------------------------------------------
// Pageable host memory is staged by the runtime and the two PCIe directions do not overlap (tools/h2d_bench.hip:
// 9.7 ms for 2 x 256 MiB whatever the threading); arrays allocated with ndfft_host_alloc are pinned, their copies
// are real DMA and the directions overlap (5.6 ms).  A dense C-layout call whose slowest dimension is a batch
// dimension is therefore split into row chunks: chunk c+1 uploads while chunk c transforms and chunk c-1 downloads.
bool is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// ---- registration cache for the caller's own (pageable) arrays ---------------------------------------------------------
// The reference's signature hands over ndarrays in ordinary host memory (src/lib.rs:105-115).  Pinned memory moves at the PCIe duplex
// rate (2 x 256 MiB: 6.2 ms through the chunk pipeline) but hipHostRegister costs ~22 ms per 512 MiB, pageable memory goes through bounce
// buffers (8-10 ms: the host memcpys bound it on a 16-CPU quota).  A caller that transforms the SAME arrays again and again -- a time
// stepper, the reference's own benches -- should pay the registration once: the SECOND time a range is seen it is registered and kept in an
// LRU, from then on its calls run the pinned pipeline.  One-shot arrays never pay.
// OPT-IN (ndfft_host_reg_cache / NDFFT_HOST_REG_CACHE_MB, default 0 = off), because a registration outlives the array: when the caller
// frees a registered array and the allocator hands the addresses out again, HIP still treats them as the old pinned object and EVERY copy
// from or to them -- this library's, torch's, the caller's own -- fails with "invalid argument" or aborts inside the HIP runtime (both seen
// on the MI355X with numpy arrays in the first version, which had the cache on by default).  This library recovers from the error form
// (it forgets the range and retries through the bounce buffers) but cannot protect other code nor survive the abort, so only a caller that
// owns its arrays' lifetimes should switch it on, and it must call ndfft_host_forget before freeing them.
class HostRegCache {
  public:
    static HostRegCache &get() { static HostRegCache *c = new HostRegCache; return *c; }
    // true: [p, p + bytes) lies inside a registration THIS CACHE owns, and is held until release(): its LRU stamp is fresh and neither
    // eviction, forget() nor set_limit(0) will unregister it while the call's copies are in flight.  Asked BEFORE is_pinned() (round 4: a
    // registered array looks like any pinned one to hipPointerGetAttributes, and the steady-state calls used to bypass the cache -- the
    // hottest arrays were evicted first, nothing held them during the DMA, and a stale registration was not retried).
    // Two steps (round 5, advisor): lookup() only consults the registrations this cache owns; sight() records a sighting of a range and registers it
    // on the second one.  HostPin calls sight() only for memory that is NOT pinned already: an ndfft_host_alloc / hipHostMalloc array that missed the
    // lookup is the caller's own pinned memory -- registering it again would either fail every time or leave the cache owning (and later
    // unregistering) a registration over memory the caller frees with hipHostFree.
    bool lookup(const void *p, size_t bytes) {
        const uintptr_t lo = (uintptr_t)p, hi = lo + std::max<size_t>(bytes, 1);
        std::lock_guard<std::mutex> g(mu_);
        ++tick_;
        for (R &r : v_) if (r.registered && r.lo <= lo && hi <= r.hi) { r.last = tick_; ++r.inuse; return true; }   // any size: sub-views of a registered array too
        return false;
    }
    bool wants(size_t bytes) { std::lock_guard<std::mutex> g(mu_); return limit_ && bytes >= ((size_t)8 << 20); }
    bool sight(const void *p, size_t bytes) {
        const uintptr_t lo = (uintptr_t)p, hi = lo + std::max<size_t>(bytes, 1);
        std::lock_guard<std::mutex> g(mu_);
        ++tick_;
        if (!limit_ || bytes < ((size_t)8 << 20)) return false;
        for (size_t i = 0; i < v_.size();) {
            R &r = v_[i];
            if (!(r.lo == lo && r.hi == hi) && lo < r.hi && r.lo < hi) {   // overlaps another range: the caller's allocation changed (an unregistered sighting
                if (r.inuse) return false;                                //   of a larger, older array must not be what gets pinned -- only the range of THIS call is)
                drop(i);
                continue;
            }
            ++i;
        }
        R *hit = nullptr;                                 // (looked up after the erasures above: they move entries)
        for (R &r : v_) if (r.lo == lo && r.hi == hi) { hit = &r; break; }
        if (hit) {
            hit->last = tick_;
            if (++hit->seen < 2) return false;            // (after a failed registration `seen` restarts at -8: a bounded back-off, not a ban)
            if (hipHostRegister((void *)lo, hi - lo, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); hit->seen = -8; return false; }
            hit->registered = true; hit->inuse = 1; reg_bytes_ += hi - lo;
            evict(lo);                                    // (evict() may move entries: `hit` is dead from here)
            return true;
        }
        if (v_.size() >= 256) {                           // forget the oldest unregistered sighting
            size_t o = v_.size();
            for (size_t i = 0; i < v_.size(); ++i) if (!v_[i].registered && (o == v_.size() || v_[i].last < v_[o].last)) o = i;
            if (o < v_.size()) v_.erase(v_.begin() + o);
        }
        v_.push_back({lo, hi, tick_, 1, false, 0});
        return false;
    }
    void release(const void *p) {
        const uintptr_t a = (uintptr_t)p;
        std::lock_guard<std::mutex> g(mu_);
        for (R &r : v_) if (r.registered && r.lo <= a && a < r.hi && r.inuse > 0) { --r.inuse; return; }
    }
    // p == nullptr: everything.  Returns the number of registrations given back.
    int forget(const void *p) {
        const uintptr_t a = (uintptr_t)p;
        std::lock_guard<std::mutex> g(mu_);
        int n = 0;
        for (size_t i = 0; i < v_.size();) {
            if ((!p || (v_[i].lo <= a && a < v_[i].hi)) && !v_[i].inuse) { n += v_[i].registered; drop(i); } else ++i;
        }
        return n;
    }
  private:
    struct R { uintptr_t lo, hi; uint64_t last; int seen; bool registered; int inuse; };
    HostRegCache() { limit_ = (size_t)std::max(0L, sw().host_reg_cache_mb) << 20; }
  public:
    void set_limit(size_t bytes) {
        std::lock_guard<std::mutex> g(mu_);
        limit_ = bytes;
        if (!bytes) { for (size_t i = 0; i < v_.size();) { if (!v_[i].inuse) drop(i); else ++i; } }
        else evict(0);
    }
  private:
    void drop(size_t i) {
        if (v_[i].registered) { (void)hipHostUnregister((void *)v_[i].lo); (void)hipGetLastError(); reg_bytes_ -= v_[i].hi - v_[i].lo; }
        v_.erase(v_.begin() + i);
    }
    void evict(uintptr_t keep) {
        while (reg_bytes_ > limit_) {
            size_t o = v_.size();
            for (size_t i = 0; i < v_.size(); ++i)
                if (v_[i].registered && !v_[i].inuse && v_[i].lo != keep && (o == v_.size() || v_[i].last < v_[o].last)) o = i;
            if (o == v_.size()) return;
            drop(o);
        }
    }
    std::mutex mu_;
    std::vector<R> v_;
    uint64_t tick_ = 0;
    size_t reg_bytes_ = 0, limit_ = 0;
};
struct HostPin {       // one side of a call: registered for the duration of the call if the cache says so
    const void *p = nullptr; bool held = false;
    HostPin(const void *ptr, size_t bytes) : p(ptr) {
        HostRegCache &c = HostRegCache::get();
        held = c.lookup(ptr, bytes);
        if (!held && c.wants(bytes) && !is_pinned(ptr)) held = c.sight(ptr, bytes);
    }
    void release() { if (held) HostRegCache::get().release(p); held = false; }
    ~HostPin() { release(); }
};
int pipe_init(Pipe &p, int chunks) {
    if (!p.ok) {
        NDFFT_HIP(hipStreamCreate(&p.h2d)); NDFFT_HIP(hipStreamCreate(&p.cmp)); NDFFT_HIP(hipStreamCreate(&p.d2h));
        p.ok = true;
    }
    while ((int)p.up.size() < chunks) {
        hipEvent_t a, b, c;
        NDFFT_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming)); NDFFT_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        NDFFT_HIP(hipEventCreateWithFlags(&c, hipEventDisableTiming));
        p.up.push_back(a); p.done.push_back(b); p.down.push_back(c);
    }
    return NDFFT_OK;
}
// span (in elements) of one index of dimension 0, i.e. of the sub-view shape[1:], or -1 if it has negative strides
int64_t inner_span(int ndim, const int64_t *shape, const int64_t *stride) {
    int64_t hi = 0;
    for (int d = 1; d < ndim; ++d) {
        if (shape[d] <= 0) return 0;
        if (stride[d] < 0) return -1;
        hi += (shape[d] - 1) * stride[d];
    }
    return hi + 1;
}
}  // namespace

// ---- pageable host arrays: the same chunk pipeline through pinned bounce buffers --------------------------------
// hipMemcpy from / to pageable memory is staged by the runtime on one thread, and the two PCIe directions never overlap
// (tools/h2d_bench.hip: 9.7 ms for 2 x 256 MiB).  Here the staging is ours: a small pool of host threads copies row
// chunks between the caller's arrays and three pinned slots per direction while the DMA engines move the previous
// chunks, so upload, transform and download overlap for ANY host array (ndarray allocates pageable memory).
namespace {
// Bulk host copy with streaming (non-temporal) stores: the pieces the pool moves (a few MiB each) are below glibc's own non-temporal threshold, so plain
// memcpy reads the destination lines before overwriting them (three memory transfers per byte instead of two).  AVX2 only where the CPU has it;
// (-DNDFFT_NO_NT_COPY keeps memcpy).  Host code only.
#if defined(__x86_64__) && !defined(NDFFT_NO_NT_COPY)
__attribute__((target("avx2"))) void copy_nt_avx2(char *d, const char *s, size_t n) {
    while (n && ((uintptr_t)d & 31)) { *d++ = *s++; --n; }
    size_t k = n / 128;
    for (; k; --k, d += 128, s += 128) {
        const __m256i a = _mm256_loadu_si256((const __m256i *)s), b = _mm256_loadu_si256((const __m256i *)(s + 32));
        const __m256i c = _mm256_loadu_si256((const __m256i *)(s + 64)), e = _mm256_loadu_si256((const __m256i *)(s + 96));
        _mm256_stream_si256((__m256i *)d, a); _mm256_stream_si256((__m256i *)(d + 32), b);
        _mm256_stream_si256((__m256i *)(d + 64), c); _mm256_stream_si256((__m256i *)(d + 96), e);
    }
    _mm_sfence();
    n &= 127;
    if (n) memcpy(d, s, n);
}
void bulk_copy(char *d, const char *s, size_t n) {
    static const bool nt = __builtin_cpu_supports("avx2");
    if (nt && n >= ((size_t)256 << 10)) copy_nt_avx2(d, s, n); else memcpy(d, s, n);
}
#else
void bulk_copy(char *d, const char *s, size_t n) { memcpy(d, s, n); }
#endif
struct CopyGroup { std::atomic<int> left{0}; std::mutex m; std::condition_variable cv; };
class CopyPool {
  public:
    static CopyPool &get() { static CopyPool *p = new CopyPool; return *p; }   // never destroyed: detached workers
    int threads() const { return nthreads_; }
    // copies `bytes` in `pieces` slices on the pool; returns immediately
    void copy_async(CopyGroup &g, char *dst, const char *src, size_t bytes, int pieces) {
        pieces = (int)std::max<size_t>(1, std::min<size_t>((size_t)pieces, bytes / (256 << 10) + 1));
        g.left.store(pieces);
        const size_t per = (bytes / pieces + 63) & ~(size_t)63;
        std::lock_guard<std::mutex> lk(mu_);
        for (int i = 0; i < pieces; ++i) {
            const size_t o = std::min(bytes, (size_t)i * per), e = i + 1 == pieces ? bytes : std::min(bytes, (size_t)(i + 1) * per);
            q_.push_back({dst + o, src + o, e - o, &g});
        }
        cv_.notify_all();
    }
    static void wait(CopyGroup &g) {
        std::unique_lock<std::mutex> lk(g.m);
        g.cv.wait(lk, [&] { return g.left.load() == 0; });
    }
  private:
    struct Piece { char *d; const char *s; size_t n; CopyGroup *g; };
    CopyPool() {
        // threads: three quarters of the CPUs this process may use (affinity / hardware count capped by the cgroup quota:
        // the MI355X boxes show 256 CPUs and grant 16), between 2 and 12.  Measured on 4096 x 4096 c128 (2 x 256 MiB,
        // plain path 9.8 ms): 4 threads 9.5-10.6 ms, 8 threads 8.8 ms, 12 threads 7.9-8.4 ms -- the host copies, not PCIe, bound it
        const int forced = sw().copy_threads;            // NDFFT_COPY_THREADS
        long hw = (long)std::thread::hardware_concurrency();
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0}; long per = 0;
            if (fscanf(f, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) hw = std::min(hw, std::max(1L, (atol(q) + per - 1) / per));
            fclose(f);
        }
        nthreads_ = forced > 0 ? forced : (int)std::max(2L, std::min(12L, hw * 3 / 4));
        if (nthreads_ < 1) nthreads_ = 1;
        for (int i = 0; i < nthreads_; ++i) std::thread([this] { loop(); }).detach();
    }
    void loop() {
        for (;;) {
            Piece p;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return !q_.empty(); });
                p = q_.front(); q_.pop_front();
            }
            bulk_copy(p.d, p.s, p.n);
            // the count changes only under the group's mutex: a waiter (whose CopyGroup lives on its stack) cannot see zero, return and
            // destroy the group while this thread is still about to lock it
            { std::lock_guard<std::mutex> lk(p.g->m); if (p.g->left.fetch_sub(1) == 1) p.g->cv.notify_all(); }
        }
    }
    int nthreads_ = 1;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Piece> q_;
};
}  // namespace

namespace {
// one ndfft_exec call after validation: what every strategy below needs, built once
struct HostCall {
    const ndfft_plan *plan; int op, ndim;
    const int64_t *shape_in, *stride_in, *shape_out, *stride_out;
    int axis, norm; double scale;
    Problem P;                   // the whole call, prepared
    DeviceWs &ws;
    size_t ein = 0, eout = 0;    // element sizes
    const char *hin = nullptr; char *hout = nullptr;   // lowest address each view touches, ilo / olo elements from element 0
    int64_t ilo = 0, olo = 0;
    size_t ibytes = 0, obytes = 0;                     // the views' spans
    bool out_dense = false;      // the output view owns every element of its span
    char *out0() const { return hout - olo * (int64_t)eout; }   // element 0 of the output view
};

// The chunk pipeline of both modes: dimension 0 cut into `chunks` row ranges, chunk c+1 uploads while chunk c transforms and chunk c-1
// downloads.  Direct mode (pinned or registered arrays) copies straight between the caller's arrays and the staging buffers; bounce mode
// (pageable arrays) goes through three pinned slots per direction that the copy pool fills and empties, downloads lagging two iterations.
int chunk_pipeline_body(HostCall &k, int chunks, bool bounce) {
    int rc;
    DeviceWs &ws = k.ws;
    Pipe &pp = ws.pipe;
    if ((rc = pipe_init(pp, chunks))) return rc;
    const int64_t R = k.shape_in[0];
    const int64_t isp = inner_span(k.ndim, k.shape_in, k.stride_in), osp = inner_span(k.ndim, k.shape_out, k.stride_out);
    struct Chunk { int64_t rows; size_t off_in, off_out, bytes_in, bytes_out; };
    auto chunk_of = [&](int c) -> Chunk {
        const int64_t r0 = R * c / chunks, n = R * (c + 1) / chunks - r0;
        if (c < 0 || c >= chunks || n <= 0) return {0, 0, 0, 0, 0};
        return {n, (size_t)(r0 * k.stride_in[0]) * k.ein, (size_t)(r0 * k.stride_out[0]) * k.eout,
                (size_t)((n - 1) * k.stride_in[0] + isp) * k.ein, (size_t)((n - 1) * k.stride_out[0] + osp) * k.eout};
    };
    CopyPool *pool = nullptr;
    int half = 1;
    if (bounce) {
        pool = &CopyPool::get();
        half = std::max(1, pool->threads() / 2);
        size_t max_in = 0, max_out = 0;
        for (int c = 0; c < chunks; ++c) { max_in = std::max(max_in, chunk_of(c).bytes_in); max_out = std::max(max_out, chunk_of(c).bytes_out); }
        for (int s = 0; s < 3; ++s) { if ((rc = ws.bounce_in[s].reserve(max_in)) || (rc = ws.bounce_out[s].reserve(max_out))) return rc; }
    }
    std::vector<int64_t> si(k.shape_in, k.shape_in + k.ndim), so(k.shape_out, k.shape_out + k.ndim);
    CopyGroup gu, gd;
    const int lag = bounce ? 2 : 0;
    for (int it = 0; it < chunks + lag; ++it) {
        const Chunk u = chunk_of(it);                                    // the chunk to upload and transform
        const bool up = u.rows > 0;
        const char *src = k.hin + u.off_in;                              // host side of its upload and download: the caller's arrays ...
        char *dst = k.hout + u.off_out;
        if (bounce) {                                                    // ... or its slots, filled / emptied by the pool
            const int cu = it, cd = it - lag;
            const Chunk d = chunk_of(cd);
            const bool dn = d.rows > 0;
            // (both waits BEFORE any pool copy is submitted: an error return must never leave the pool working on gu / gd)
            if (up && cu >= 3) NDFFT_HIP(hipEventSynchronize(pp.up[cu - 3]));      // the slot's previous upload has left it
            if (dn) NDFFT_HIP(hipEventSynchronize(pp.down[cd]));                    // chunk cd has arrived in its slot
            if (up) pool->copy_async(gu, (char *)ws.bounce_in[cu % 3].p, src, u.bytes_in, half);
            if (dn) pool->copy_async(gd, k.hout + d.off_out, (const char *)ws.bounce_out[cd % 3].p, d.bytes_out, half);
            if (up) CopyPool::wait(gu);
            if (dn) CopyPool::wait(gd);
            src = (const char *)ws.bounce_in[cu % 3].p; dst = (char *)ws.bounce_out[cu % 3].p;
        }
        if (!up) continue;
        NDFFT_HIP(hipMemcpyAsync((char *)ws.stage_in.p + u.off_in, src, u.bytes_in, hipMemcpyHostToDevice, pp.h2d));
        NDFFT_HIP(hipEventRecord(pp.up[it], pp.h2d));
        NDFFT_HIP(hipStreamWaitEvent(pp.cmp, pp.up[it], 0));
        si[0] = so[0] = u.rows;
        Problem P;
        bool nothing;
        if ((rc = prepare(k.plan, k.op, k.ndim, si.data(), k.stride_in, so.data(), k.stride_out, k.axis, k.norm, k.scale, P, nothing))) return rc;
        if (!nothing && (rc = dispatch_peeled(P, (const char *)ws.stage_in.p + u.off_in, (char *)ws.stage_out.p + u.off_out, k.ein, k.eout, pp.cmp))) return rc;
        NDFFT_HIP(hipEventRecord(pp.done[it], pp.cmp));
        NDFFT_HIP(hipStreamWaitEvent(pp.d2h, pp.done[it], 0));
        NDFFT_HIP(hipMemcpyAsync(dst, (const char *)ws.stage_out.p + u.off_out, u.bytes_out, hipMemcpyDeviceToHost, pp.d2h));
        if (bounce) NDFFT_HIP(hipEventRecord(pp.down[it], pp.d2h));     // (bounce mode ends on the last of these, waited for above)
    }
    if (!bounce) {
        NDFFT_HIP(hipStreamSynchronize(pp.d2h));
        NDFFT_HIP(hipStreamSynchronize(pp.cmp));
    }
    return NDFFT_OK;
}
int chunk_pipeline(HostCall &k, int chunks, bool bounce) {
    const int rc = chunk_pipeline_body(k, chunks, bounce);
    // on an error some chunks' asynchronous copies into the caller's arrays (and into the staging buffers, which the
    // next call may regrow) are still in flight: never return before they have drained
    // (pool copies are always waited for inside the body; only device work can be in flight)
    if (rc) k.ws.pipe.sync_all();
    return rc;
}

// "A chunk pipeline is possible for this call": dense, C-ordered in dimension 0, transform along another axis
bool can_pipeline(const HostCall &k) {
    if (!(k.ndim >= 2 && k.axis != 0 && k.ilo == 0 && k.olo == 0 && k.shape_in[0] == k.shape_out[0] && k.shape_in[0] >= 16 &&
          k.out_dense && k.ibytes + k.obytes >= ((size_t)8 << 20))) return false;
    const int64_t isp = inner_span(k.ndim, k.shape_in, k.stride_in), osp = inner_span(k.ndim, k.shape_out, k.stride_out);
    return isp > 0 && osp > 0 && k.stride_in[0] >= isp && k.stride_out[0] >= osp;
}
// a chunk must stay a real problem: kernel choice depends on the size of a call (hiprtc specialisation from 2^16-2^17
// points), so never cut below 2^18 points per chunk
int64_t max_chunks(const HostCall &k) { return std::max<int64_t>(1, (k.P.nlanes * std::max(k.P.xlen, k.P.ylen)) >> 18); }

// ---- the strategies, in order of preference: each returns NDFFT_OK, a real error, or kDeclined ---------------------------------------

// Small calls (the reference's own bench shapes: benches/ndrustfft.rs:6-7, n x n with n = 128 ... 264): no DMA at all.  The kernels read the
// input straight from a pinned, device-mapped bounce buffer over PCIe and write the output into another one: two host memcpys and ONE stream
// synchronisation are the whole call (the plain path below pays two synchronous hipMemcpy of pageable memory, ~15-20 us each whatever the size).
int host_small(HostCall &k) {
    const size_t small_limit = (size_t)NDFFT_DEV_INT("NDFFT_HOST_SMALL_KB", 2048) << 10;
    if (k.ibytes + k.obytes > small_limit) return kDeclined;
    DeviceWs &ws = k.ws;
    int rc;
    if ((rc = ws.bounce_in[0].reserve(std::max(k.ibytes, small_limit))) || (rc = ws.bounce_out[0].reserve(std::max(k.obytes, small_limit)))) return rc;
    memcpy(ws.bounce_in[0].p, k.hin, k.ibytes);
    const char *din = (const char *)ws.bounce_in[0].p - k.ilo * (int64_t)k.ein;
    char *dout = (char *)ws.bounce_out[0].p - k.olo * (int64_t)k.eout;
    rc = dispatch_peeled(k.P, din, dout, k.ein, k.eout, (hipStream_t) nullptr);
    const hipError_t se = hipStreamSynchronize(nullptr);
    if (rc) return rc;
    if (se != hipSuccess) return fail(NDFFT_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    if (k.out_dense) memcpy(k.hout, ws.bounce_out[0].p, k.obytes);
    else copy_view_elements(k.out0(), dout, k.ndim, k.shape_out, k.stride_out, k.eout);   // holes belong to the caller
    return NDFFT_OK;
}

// pipelined row chunks, straight DMA: the caller's pinned arrays (ndfft_host_alloc), or its own arrays, seen before: registered once, DMA
// straight from / to them from then on.  The cache is asked FIRST (held = a registration it owns, kept alive for this call); only an array
// it does not own can be the caller's pinned memory
int host_pinned(HostCall &k) {
    if (!can_pipeline(k)) return kDeclined;
    HostPin pin_in(k.hin, k.ibytes), pin_out(k.hout, k.obytes);
    const bool own_in = !pin_in.held && is_pinned(k.hin), own_out = !pin_out.held && is_pinned(k.hout);
    if (!((own_in || pin_in.held) && (own_out || pin_out.held))) return kDeclined;
    const int chunks = (int)std::min<int64_t>(std::min<int64_t>(k.shape_in[0], max_chunks(k)), 8);
    const int rc = chunk_pipeline(k, chunks, false);
    // A registration made by the cache can be stale: the caller freed the array and the allocator handed the same addresses out
    // again (seen on the MI355X with numpy arrays: hipMemcpyAsync then fails with "invalid argument" -- before anything has been
    // written to the caller's output).  Forget both ranges and run this call through the bounce buffers instead.
    if (rc != NDFFT_ERR_HIP || !(pin_in.held || pin_out.held)) return rc;
    pin_out.release(); pin_in.release();              // (a range that is still held is not forgotten)
    (void)hipGetLastError();
    HostRegCache::get().forget(k.hin); HostRegCache::get().forget(k.hout);
    clear_err();
    return kDeclined;
}

// pipelined row chunks through pinned bounce buffers filled by the copy pool, for pageable arrays.  NDFFT_HOST_PIPE=0: plain path.
int host_bounce(HostCall &k) {
    if (!can_pipeline(k)) return kDeclined;
    const int hp = sw().host_pipe;                    // NDFFT_HOST_PIPE
    const bool force = hp == 1;                       // tests: pipeline small calls too
    if (!(force || (hp != 0 && max_chunks(k) >= 4 && k.ibytes + k.obytes >= ((size_t)32 << 20)))) return kDeclined;   // small calls: the plain path
    // chunks of ~32 MiB per direction (at least 4, at most 64)
    const int64_t want = std::max<int64_t>(4, std::min<int64_t>(64, (int64_t)(std::max(k.ibytes, k.obytes) >> 25)));
    const int chunks = (int)std::min<int64_t>(std::min<int64_t>(k.shape_in[0], force ? 64 : max_chunks(k)), want);
    return chunk_pipeline(k, chunks, true);
}

// (a copy that fails may have met a stale cached registration over the caller's array -- see HostRegCache: forget it and try once more)
int copy_host(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const void *host_side) {
    if (hipMemcpy(dst, src, bytes, kind) == hipSuccess) return NDFFT_OK;
    (void)hipGetLastError();
    if (!HostRegCache::get().forget(host_side)) return fail(NDFFT_ERR_HIP, "hipMemcpy between the caller's array and the device failed");
    NDFFT_HIP(hipMemcpy(dst, src, bytes, kind));
    return NDFFT_OK;
}
// everything else: two synchronous copies around the transform on the null stream
int host_plain(HostCall &k) {
    DeviceWs &ws = k.ws;
    int rc;
    if (!k.out_dense && (rc = ws.bounce_out[0].reserve(k.obytes))) return rc;   // before anything is in flight
    if ((rc = copy_host(ws.stage_in.p, k.hin, k.ibytes, hipMemcpyHostToDevice, k.hin))) return rc;
    const char *din = (const char *)ws.stage_in.p - k.ilo * (int64_t)k.ein;
    char *dout = (char *)ws.stage_out.p - k.olo * (int64_t)k.eout;
    rc = dispatch_peeled(k.P, din, dout, k.ein, k.eout, (hipStream_t) nullptr);
    if (rc) { (void)hipStreamSynchronize(nullptr); return rc; }
    if (k.out_dense) return copy_host(k.hout, ws.stage_out.p, k.obytes, hipMemcpyDeviceToHost, k.hout);   // synchronises with the kernel
    // The output view has holes.  They belong to the caller (possibly to ANOTHER thread's &mut view of the same
    // allocation), so they are neither read nor written: the span comes back into a private pinned image and only
    // the view's own elements are copied out of it.
    NDFFT_HIP(hipMemcpy(ws.bounce_out[0].p, ws.stage_out.p, k.obytes, hipMemcpyDeviceToHost));
    copy_view_elements(k.out0(), (const char *)ws.bounce_out[0].p - k.olo * (int64_t)k.eout, k.ndim, k.shape_out, k.stride_out, k.eout);
    return NDFFT_OK;
}
}  // namespace

extern "C" {

int ndfft_host_alloc(void **h_ptr, size_t bytes) {
    clear_err();
    if (!h_ptr) return fail(NDFFT_ERR_INVALID_ARG, "h_ptr is null");
    NDFFT_HIP(hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return NDFFT_OK;
}
int ndfft_host_free(void *h_ptr) {
    clear_err();
    if (h_ptr) NDFFT_HIP(hipHostFree(h_ptr));
    return NDFFT_OK;
}

int ndfft_exec(const ndfft_plan *plan, int op, const void *in, void *out, int ndim, const int64_t *shape_in,
               const int64_t *stride_in, const int64_t *shape_out, const int64_t *stride_out, int axis, int norm,
               double scale) {
    clear_err();
    Problem P;
    bool nothing;
    int rc = prepare(plan, op, ndim, shape_in, stride_in, shape_out, stride_out, axis, norm, scale, P, nothing);
    if (rc || nothing) return rc;
    if (!in || !out) return fail(NDFFT_ERR_INVALID_ARG, "null array pointer");
    DeviceWs *ws;
    if ((rc = current_ws(&ws))) return rc;
    HostCall k{plan, op, ndim, shape_in, stride_in, shape_out, stride_out, axis, norm, scale, std::move(P), *ws};
    const size_t r = real_size(plan->dtype);
    k.ein = op_in_cplx(op) ? 2 * r : r; k.eout = op_out_cplx(op) ? 2 * r : r;
    int64_t ihi, icnt, ohi, ocnt;
    view_range(ndim, shape_in, stride_in, k.ilo, ihi, icnt);
    view_range(ndim, shape_out, stride_out, k.olo, ohi, ocnt);
    k.ibytes = (size_t)(ihi - k.ilo + 1) * k.ein; k.obytes = (size_t)(ohi - k.olo + 1) * k.eout;
    k.hin = (const char *)in + k.ilo * (int64_t)k.ein;
    k.hout = (char *)out + k.olo * (int64_t)k.eout;
    k.out_dense = (int64_t)(ohi - k.olo + 1) == ocnt;
    // the strategies in order of preference; plain synchronous copies take whatever none of the others does
    if ((rc = host_small(k)) != kDeclined) return rc;
    if ((rc = ws->stage_in.reserve(k.ibytes)) || (rc = ws->stage_out.reserve(k.obytes))) return rc;   // every strategy below stages through these
    if ((rc = host_pinned(k)) != kDeclined) return rc;
    if ((rc = host_bounce(k)) != kDeclined) return rc;
    return host_plain(k);
}

int ndfft_host_reg_cache(size_t max_bytes) {
    clear_err();
    HostRegCache::get().set_limit(max_bytes);
    return NDFFT_OK;
}

int ndfft_host_forget(const void *h_ptr) {
    clear_err();
    (void)HostRegCache::get().forget(h_ptr);
    return NDFFT_OK;
}

}  // extern "C"
