// ndfft_filter in the C++ mirror (include/ndrustfft.hpp) along axis 0 of C-layout DeviceArrays -- the column form of the fused kernel, path filter_col_pow2 --
// against the three calls it stands for (ndfft, a multiply on the host, ndifft through the same mirror): fused, composed on request, in place.
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
static double max_diff(const std::vector<C> &a, const std::vector<C> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300;
    for (std::size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::abs(a[i] - b[i]));
    return m;
}

// the three calls on the host path along axis 0, the multiply on the host in between
static std::vector<C> three_calls(const Array<C> &x, const FftHandler<double> &h, const std::vector<C> &w) {
    const auto shape = x.shape();
    auto s = Array<C>::zeros(shape), y = Array<C>::zeros(shape);
    ndfft(x, s, h, 0);
    auto v = s.to_logical();
    const std::int64_t inner = shape[1], n = shape[0];
    for (std::size_t i = 0; i < v.size(); ++i) v[i] *= w[(std::size_t)(((std::int64_t)i / inner) % n)];
    ndifft(Array<C>::from(shape, v), y, h, 0);
    return y.to_logical();
}

static void col(std::int64_t n, std::int64_t inner) {
    std::vector<C> in; for (int i = 0; i < n * inner; ++i) in.emplace_back(std::sin(0.31 * i), std::cos(0.17 * i) + 1e-3 * (i % 97));
    auto x = Array<C>::from({n, inner}, in);
    auto h = FftHandler<double>((std::size_t)n);
    const auto w = wc((std::size_t)n);
    const auto ref = three_calls(x, h, w);
    double scale = 0; for (const C &v : ref) scale = std::fmax(scale, std::abs(v));
    auto dw = DeviceArray<C>::from_host(Array<C>::from({n}, w));
    auto dx = DeviceArray<C>::from_host(x); DeviceArray<C> dy({n, inner});
    ndfft_filter(dx, dy, h, 0, dw);
    EXPECT(std::string(ndfft_last_path()) == "filter_col_pow2");
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12 * scale);
    EXPECT(max_diff(dx.to_host().to_logical(), x.to_logical()) == 0.0);       // the caller's input is not written
    ndfft_filter(dx, dy, h, 0, dw, false);                                      // the composed form on request
    EXPECT(std::string(ndfft_last_path()).find("+weights+") != std::string::npos);
    EXPECT(max_diff(dy.to_host().to_logical(), ref) < 1e-12 * scale);
    ndfft_filter(dx, dx, h, 0, dw);                                             // in place
    EXPECT(std::string(ndfft_last_path()) == "filter_col_pow2");
    EXPECT(max_diff(dx.to_host().to_logical(), ref) < 1e-12 * scale);
}

int main() {
    try {
        col(256, 40);
        col(1024, 12);         // (a radix list that is no palindrome: the second twiddle table; tiles of 8 lanes: a ragged second tile)
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) { std::printf("test result: FAILED. %d failed\n", failures); return 1; }
    std::printf("test result: ok.\n");
    return 0;
}
