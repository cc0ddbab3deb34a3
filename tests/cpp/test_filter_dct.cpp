// nddct_filter on DeviceArrays in the C++ mirror (include/ndrustfft.hpp) against the three calls it stands for -- nddct2, a multiply on the host, nddct3 through the
// same mirror -- on fused shapes (path filter_dct_pow2), composed ones, the composed form on request, and in place.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ndrustfft.hpp"

using namespace ndrustfft;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static std::vector<double> wr(std::size_t n) { std::vector<double> w(n); for (std::size_t j = 0; j < n; ++j) w[j] = (j % 3 ? 1.0 : -1.0) * (0.5 + std::fmod(0.37 * (double)j, 1.5)); return w; }
static double max_rel(const std::vector<double> &a, const std::vector<double> &b) {
    double m = a.size() == b.size() ? 0.0 : 1e300, s = 1e-300;
    for (std::size_t i = 0; i < b.size(); ++i) s = std::fmax(s, std::abs(b[i]));
    for (std::size_t i = 0; i < a.size() && i < b.size(); ++i) m = std::fmax(m, std::abs(a[i] - b[i]) / s);
    return m;
}

// want: the fused path's name, or nullptr for a composed one
static void dct(std::int64_t nx, std::int64_t ny, std::size_t axis, const char *want, bool none = false) {
    std::vector<double> in; for (int i = 0; i < nx * ny; ++i) in.push_back(std::sin(0.31 * i) + 1e-3 * (i % 89));
    auto x = Array<double>::from({nx, ny}, in);
    const std::size_t n = (std::size_t)(axis == 0 ? nx : ny);
    auto h = DctHandler<double>(n);
    if (none) h = DctHandler<double>(n).normalization(Normalization<double>::none());
    const auto w = wr(n);
    auto c = Array<double>::zeros({nx, ny}); auto y = Array<double>::zeros({nx, ny});
    nddct2(x, c, h, axis);
    auto v = c.to_logical();
    const std::int64_t inner = axis == 0 ? ny : 1;
    for (std::size_t i = 0; i < v.size(); ++i) v[i] *= w[(std::size_t)(((std::int64_t)i / inner) % (std::int64_t)n)];
    nddct3(Array<double>::from({nx, ny}, v), y, h, axis);
    const auto ref = y.to_logical();
    auto dw = DeviceArray<double>::from_host(Array<double>::from({(std::int64_t)w.size()}, w));
    auto dx = DeviceArray<double>::from_host(x); DeviceArray<double> dy({nx, ny});
    nddct_filter(dx, dy, h, axis, dw);
    const std::string path = ndfft_last_path();
    EXPECT(want ? path == want : path.find("+weights+") != std::string::npos);
    EXPECT(max_rel(dy.to_host().to_logical(), ref) < 1e-12);
    EXPECT(max_rel(dx.to_host().to_logical(), x.to_logical()) == 0.0);         // the caller's input is not written
    nddct_filter(dx, dy, h, axis, dw, false);                                   // the composed form on request
    EXPECT(std::string(ndfft_last_path()).find("+weights+") != std::string::npos);
    EXPECT(max_rel(dy.to_host().to_logical(), ref) < 1e-12);
    nddct_filter(dx, dx, h, axis, dw);                                          // in place
    EXPECT(std::string(ndfft_last_path()) == path);
    EXPECT(max_rel(dx.to_host().to_logical(), ref) < 1e-12);
}

int main() {
    try {
        dct(37, 256, 1, "filter_dct_pow2");
        dct(5, 2048, 1, "filter_dct_pow2");            // (a radix list that is no palindrome: the second twiddle table)
        dct(5, 512, 1, "filter_dct_pow2", true);       // Normalization::None
        dct(5, 64, 1, nullptr);
        dct(128, 6, 0, nullptr);                        // strided lanes of a fused length
        dct(6, 96, 1, nullptr);
    } catch (const std::exception &e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    if (failures) { std::printf("test result: FAILED. %d failed\n", failures); return 1; }
    std::printf("test result: ok.\n");
    return 0;
}
