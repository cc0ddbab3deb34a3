// Normalization::weights in the C++ mirror (include/ndrustfft.hpp): the host path (one multiply around ndfft_exec) and the DeviceArray path
// (ndfft_exec_weighted_device, the vector uploaded once into a buffer the Normalization owns) against the equivalent Normalization::custom
// function, for ndifft (after, on the output lane) and nddct1 (before, on the input lane), along both axes of a 2-D array.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ndrustfft.hpp"

using namespace ndrustfft;
typedef Complex<double> C;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static const int NX = 5, NY = 8;
static std::vector<C> wc(std::size_t n) { std::vector<C> w(n); for (std::size_t j = 0; j < n; ++j) w[j] = C(0.5 + 0.25 * (double)j, 1.0 - 0.125 * (double)j); return w; }
static std::vector<double> wr(std::size_t n) { std::vector<double> w(n); for (std::size_t j = 0; j < n; ++j) w[j] = (j % 2 ? -1.0 : 1.0) * (0.5 + 0.1875 * (double)j); return w; }
static void fn_c(C *d, std::size_t len) { auto w = wc(len); for (std::size_t j = 0; j < len; ++j) d[j] *= w[j]; }
static void fn_r(double *d, std::size_t len) { auto w = wr(len); for (std::size_t j = 0; j < len; ++j) d[j] *= w[j]; }

template <typename A> static double max_diff(const std::vector<A> &a, const std::vector<A> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (std::size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::abs(a[i] - b[i]));
    return m;
}

static void ifft_weights() {
    std::vector<C> in; for (int i = 0; i < NX * NY; ++i) in.emplace_back(std::sin(0.31 * i), std::cos(0.17 * i) + 0.01 * i);
    auto x = Array<C>::from({NX, NY}, in);
    for (std::size_t axis = 0; axis < 2; ++axis) {
        const std::size_t n = axis == 0 ? NX : NY;
        auto hc = FftHandler<double>(n).normalization(Normalization<C>::custom(fn_c));
        auto hw = FftHandler<double>(n).normalization(Normalization<C>::weights(wc(n)));
        auto yc = Array<C>::zeros({NX, NY}), yw = Array<C>::zeros({NX, NY});
        ndifft(x, yc, hc, axis); ndifft(x, yw, hw, axis);                 // host path
        EXPECT(max_diff(yw.to_logical(), yc.to_logical()) < 1e-12);
        auto dx = DeviceArray<C>::from_host(x); DeviceArray<C> dy({NX, NY});
        ndifft(dx, dy, hw, axis);                                          // device path: the pass runs after the transform, in place on dy
        EXPECT(std::string(ndfft_last_path()).find("+weights") != std::string::npos);
        EXPECT(max_diff(dy.to_host().to_logical(), yc.to_logical()) < 1e-12);
        ndifft(dx, dy, hw, axis);                                          // the vector is uploaded once: a second call reuses it
        EXPECT(max_diff(dy.to_host().to_logical(), yc.to_logical()) < 1e-12);
        DeviceArray<C> dz({NX, NY});
        ndfft(dx, dz, hw, axis);                                           // the forward op ignores the weights
        auto yf = Array<C>::zeros({NX, NY}); ndfft(x, yf, FftHandler<double>(n), axis);
        EXPECT(max_diff(dz.to_host().to_logical(), yf.to_logical()) < 1e-12);
    }
}

static void dct1_weights() {
    std::vector<double> d(NX * NY); for (int i = 0; i < NX * NY; ++i) d[i] = std::cos(0.3 * i) + 0.1 * i;
    auto x = Array<double>::from({NX, NY}, d);
    for (std::size_t axis = 0; axis < 2; ++axis) {
        const std::size_t n = axis == 0 ? NX : NY;
        auto hc = DctHandler<double>(n).normalization(Normalization<double>::custom(fn_r));
        auto hw = DctHandler<double>(n).normalization(Normalization<double>::weights(wr(n)));
        auto yc = Array<double>::zeros({NX, NY}), yw = Array<double>::zeros({NX, NY});
        nddct1(x, yc, hc, axis); nddct1(x, yw, hw, axis);
        EXPECT(max_diff(yw.to_logical(), yc.to_logical()) < 1e-12);
        auto dx = DeviceArray<double>::from_host(x); DeviceArray<double> dy({NX, NY});
        nddct1(dx, dy, hw, axis);
        EXPECT(std::string(ndfft_last_path()).rfind("weights+", 0) == 0);
        EXPECT(max_diff(dy.to_host().to_logical(), yc.to_logical()) < 1e-12);
        EXPECT(max_diff(dx.to_host().to_logical(), x.to_logical()) == 0.0);     // the caller's input is not written
    }
    // a vector of the wrong length is refused on both paths
    auto bad = DctHandler<double>(NY).normalization(Normalization<double>::weights(wr(NY + 1)));
    auto y = Array<double>::zeros({NX, NY});
    try { nddct1(x, y, bad, 1); EXPECT(!"no error"); } catch (const Error &e) { EXPECT(e.status == NDFFT_ERR_INVALID_ARG); }
    auto dx = DeviceArray<double>::from_host(x); DeviceArray<double> dy({NX, NY});
    try { nddct1(dx, dy, bad, 1); EXPECT(!"no error"); } catch (const Error &e) { EXPECT(e.status == NDFFT_ERR_INVALID_ARG); }
    // ... and BEFORE the transform has run, also where the weights act on the output (ndifft): the output keeps its contents
    auto badc = FftHandler<double>(NY).normalization(Normalization<C>::weights(wc(NY - 1)));
    auto xc = Array<C>::zeros({NX, NY}); xc(0, 0) = C(1., 0.);
    auto yc = Array<C>::from({NX, NY}, std::vector<C>(NX * NY, C(7.25, 7.25)));
    try { ndifft(xc, yc, badc, 1); EXPECT(!"no error"); } catch (const Error &e) { EXPECT(e.status == NDFFT_ERR_INVALID_ARG); }
    for (const C &v : yc.to_logical()) EXPECT(v == C(7.25, 7.25));
    // an array of the wrong size still gets the reference's panic, not a complaint about the weights
    auto okw = FftHandler<double>(NY).normalization(Normalization<C>::weights(wc(NY)));
    auto xs = Array<C>::zeros({NX, NY - 1}), ys = Array<C>::zeros({NX, NY - 1});
    try { ndifft(xs, ys, okw, 1); EXPECT(!"no panic"); } catch (const Panic &e) { EXPECT(e.status == NDFFT_ERR_SIZE_MISMATCH); }
}

int main() {
    try {
        ifft_weights();
        dct1_weights();
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) { std::printf("test result: FAILED. %d failed\n", failures); return 1; }
    std::printf("test result: ok.\n");
    return 0;
}
