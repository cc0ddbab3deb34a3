// ndfft_filter on REAL DeviceArrays in the C++ mirror (include/ndrustfft.hpp) against the three calls it stands for -- ndfft_r2c, a multiply on the host, ndifft_r2c
// through the same mirror -- on fused shapes (path filter_r2c_pow2), composed ones, the composed form on request, and in place.
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
static double max_diff(const std::vector<double> &a, const std::vector<double> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (std::size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::abs(a[i] - b[i]));
    return m;
}

// want: the fused path's name, or nullptr for a composed one
static void r2c(std::int64_t nx, std::int64_t ny, std::size_t axis, const char *want) {
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
    const auto ref = y.to_logical();
    auto dw = DeviceArray<C>::from_host(Array<C>::from({(std::int64_t)w.size()}, w));
    auto dx = DeviceArray<double>::from_host(x); DeviceArray<double> dy({nx, ny});
    ndfft_filter(dx, dy, h, axis, dw);
    const std::string path = ndfft_last_path();
    EXPECT(want ? path == want : path.find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12);
    EXPECT(max_diff(dx.to_host().to_logical(), x.to_logical()) == 0.0);       // the caller's input is not written
    ndfft_filter(dx, dy, h, axis, dw, false);                                   // the composed form on request
    EXPECT(std::string(ndfft_last_path()).find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12);
    ndfft_filter(dx, dx, h, axis, dw);                                          // in place
    EXPECT(std::string(ndfft_last_path()) == path);
    EXPECT(max_diff(dx.to_host().to_logical(), ref) < 1e-12);
}

int main() {
    try {
        r2c(37, 256, 1, "filter_r2c_pow2");
        r2c(5, 2048, 1, "filter_r2c_pow2");            // (a radix list that is no palindrome: the second twiddle table)
        r2c(5, 64, 1, nullptr);
        r2c(128, 6, 0, nullptr);                        // strided lanes of a fused length
        r2c(6, 96, 1, nullptr);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) { std::printf("test result: FAILED. %d failed\n", failures); return 1; }
    std::printf("test result: ok.\n");
    return 0;
}
