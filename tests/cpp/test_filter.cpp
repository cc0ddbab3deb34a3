// ndfft_filter in the C++ mirror (include/ndrustfft.hpp) on DeviceArrays against the three calls it stands for -- ndfft, a multiply on the host, ndifft (and the
// R2C pair) through the same mirror -- on a fused shape, composed shapes along both axes, in place, and the refusals.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ndrustfft.hpp"

using namespace ndrustfft;
typedef Complex<double> C;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static std::vector<C> wc(std::size_t n) { std::vector<C> w(n); for (std::size_t j = 0; j < n; ++j) w[j] = C(0.5 + std::fmod(0.37 * (double)j, 1.5), 1.0 - std::fmod(0.11 * (double)j, 2.0)); return w; }
template <typename A> static double max_diff(const std::vector<A> &a, const std::vector<A> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (std::size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::abs(a[i] - b[i]));
    return m;
}
static DeviceArray<C> dev_weights(const std::vector<C> &w) { return DeviceArray<C>::from_host(Array<C>::from({(std::int64_t)w.size()}, w)); }

// the three calls on the host path, the multiply on the host in between
static std::vector<C> three_calls(const Array<C> &x, const FftHandler<double> &h, std::size_t axis, const std::vector<C> &w) {
    const auto shape = x.shape();
    auto s = Array<C>::zeros(shape), y = Array<C>::zeros(shape);
    ndfft(x, s, h, axis);
    auto v = s.to_logical();
    const std::int64_t inner = axis == 0 ? shape[1] : 1, n = shape[axis];
    for (std::size_t i = 0; i < v.size(); ++i) v[i] *= w[(std::size_t)(((std::int64_t)i / inner) % n)];
    ndifft(Array<C>::from(shape, v), y, h, axis);
    return y.to_logical();
}

static void c2c(std::int64_t nx, std::int64_t ny, std::size_t axis, bool none, const char *want) {
    std::vector<C> in; for (int i = 0; i < nx * ny; ++i) in.emplace_back(std::sin(0.31 * i), std::cos(0.17 * i) + 1e-3 * (i % 97));
    auto x = Array<C>::from({nx, ny}, in);
    const std::size_t n = (std::size_t)(axis == 0 ? nx : ny);
    auto h = FftHandler<double>(n);
    if (none) h = FftHandler<double>(n).normalization(Normalization<C>::none());
    const auto w = wc(n);
    const auto ref = three_calls(x, h, axis, w);
    double scale = 0; for (const C &v : ref) scale = std::fmax(scale, std::abs(v));
    auto dw = dev_weights(w);
    auto dx = DeviceArray<C>::from_host(x); DeviceArray<C> dy({nx, ny});
    ndfft_filter(dx, dy, h, axis, dw);
    const std::string path = ndfft_last_path();
    EXPECT(want ? path == want : path.find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12 * scale);
    EXPECT(max_diff(dx.to_host().to_logical(), x.to_logical()) == 0.0);       // the caller's input is not written
    ndfft_filter(dx, dy, h, axis, dw, false);                                   // the composed form on request
    EXPECT(std::string(ndfft_last_path()).find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12 * scale);
    ndfft_filter(dx, dx, h, axis, dw);                                          // in place
    EXPECT(std::string(ndfft_last_path()) == path);
    EXPECT(max_diff(dx.to_host().to_logical(), ref) < 1e-12 * scale);
}

static void r2c(std::int64_t nx, std::int64_t ny, std::size_t axis) {
    std::vector<double> in; for (int i = 0; i < nx * ny; ++i) in.push_back(std::sin(0.31 * i) + 1e-3 * (i % 89));
    auto x = Array<double>::from({nx, ny}, in);
    const std::size_t n = (std::size_t)(axis == 0 ? nx : ny), m = n / 2 + 1;
    auto h = R2cFftHandler<double>(n);
    const auto w = wc(m);
    std::vector<std::int64_t> sshape = {nx, ny}; sshape[axis] = (std::int64_t)m;
    auto s = Array<C>::zeros(sshape); auto y = Array<double>::zeros({nx, ny});
    ndfft_r2c(x, s, h, axis);
    auto v = s.to_logical();
    const std::int64_t inner = axis == 0 ? ny : 1;
    for (std::size_t i = 0; i < v.size(); ++i) v[i] *= w[(std::size_t)(((std::int64_t)i / inner) % (std::int64_t)m)];
    ndifft_r2c(Array<C>::from(sshape, v), y, h, axis);
    auto dw = dev_weights(w);
    auto dx = DeviceArray<double>::from_host(x); DeviceArray<double> dy({nx, ny});
    ndfft_filter(dx, dy, h, axis, dw);
    EXPECT(std::string(ndfft_last_path()).find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), y.to_logical()) < 1e-12);
}

static void refusals() {
    auto x = Array<C>::from({3, 8}, std::vector<C>(24, C(1., 0.)));
    auto dx = DeviceArray<C>::from_host(x);
    auto dy = DeviceArray<C>::from_host(Array<C>::from({3, 8}, std::vector<C>(24, C(7.25, 7.25))));
    auto h = FftHandler<double>(8);
    auto w7 = dev_weights(wc(7)), w8 = dev_weights(wc(8));
    try { ndfft_filter(dx, dy, h, 1, w7); EXPECT(!"no error"); } catch (const Error &e) { EXPECT(e.status == NDFFT_ERR_INVALID_ARG); }
    auto hw = FftHandler<double>(8).normalization(Normalization<C>::weights(wc(8)));
    try { ndfft_filter(dx, dy, hw, 1, w8); EXPECT(!"no error"); } catch (const Error &e) { EXPECT(e.status == NDFFT_ERR_INVALID_ARG); }
    try { ndfft_filter(dx, dy, FftHandler<double>(6), 1, w8); EXPECT(!"no panic"); } catch (const Panic &e) { EXPECT(e.status == NDFFT_ERR_SIZE_MISMATCH); }
    try { ndfft_filter(dx, dy, h, 2, w8); EXPECT(!"no panic"); } catch (const Panic &e) { EXPECT(e.status == NDFFT_ERR_AXIS); }
    for (const C &v : dy.to_host().to_logical()) EXPECT(v == C(7.25, 7.25));      // a refused call wrote nothing
}

int main() {
    try {
        c2c(37, 256, 1, false, "filter_pow2");
        c2c(5, 1024, 1, true, "filter_pow2");          // (a radix list that is no palindrome: the second twiddle table)
        c2c(6, 96, 1, false, nullptr);
        c2c(40, 7, 0, true, nullptr);
        r2c(5, 64, 1);
        r2c(9, 6, 0);
        refusals();
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) { std::printf("test result: FAILED. %d failed\n", failures); return 1; }
    std::printf("test result: ok.\n");
    return 0;
}
