// denoise_san_main.cpp — TEST INFRASTRUCTURE.  A stand-alone program (built
// with -fsanitize=address,undefined by this directory's Makefile, run by
// tests/test_denoise_host.py) that drives the denoiser's host tap function
// over the test shapes with every frame in an exactly-sized heap allocation:
// the clamped 3 x 3 and the skipped 5 x 5 taps at strides 1 .. 128 must never
// form an index outside the frame.
#include <math.h>
#include <stdio.h>

#include "pt_denoise_host.cpp"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double rnd() {   // xorshift64*, uniform in [0, 1)
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

static int run(int32_t W, int32_t H, int32_t iters) {
    const size_t np = (size_t)W * (size_t)H;
    std::vector<double> c(np * 3), v(np * 3), N(np * 3), P(np * 3), oc(np * 3), ov(np * 3);
    std::vector<int32_t> obj(np);
    for (int32_t row = 0; row < H; ++row)
        for (int32_t col = 0; col < W; ++col) {
            const size_t e = (size_t)row * W + col;
            obj[e] = (int32_t)(((row / 4) * 7 + (col / 4) * 3) % 5) - 1;   // 4 x 4 patches, -1 included
            const int kind = (int)(rnd() * 4.0);
            double nn[3] = {rnd() - 0.5, rnd() - 0.5, rnd() - 0.5};
            const double len = sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]) + 1e-30;
            const bool shared = rnd() < 0.7;   // unit normals: the pixel's own, or (0, 0, 1)
            for (int k = 0; k < 3; ++k) {
                c[3 * e + k] = 2.0 * rnd();
                v[3 * e + k] = kind == 0 ? 0.0 : (kind == 1 ? 1e-300 * rnd() : (kind == 2 ? 0.05 * rnd() : 1e6 * rnd()));
                N[3 * e + k] = obj[e] < 0 ? 0.0 : (shared ? (k == 2 ? 1.0 : 0.0) : nn[k] / len);
                P[3 * e + k] = obj[e] < 0 ? 0.0 : (k == 2 && rnd() < 0.5 ? -25.0 : 8.0 * rnd() - 4.0);
            }
        }
    pt_denoise_params d = {2.0, 0.1, 1e-10, iters, 5, 0};
    if (hd_denoise(W, H, &d, c.data(), v.data(), obj.data(), N.data(), P.data(), oc.data(), ov.data())) return 1;
    for (size_t i = 0; i < np * 3; ++i)
        if (!isfinite(oc[i]) || !isfinite(ov[i])) {
            fprintf(stderr, "%dx%d iters %d: element %zu is not finite\n", W, H, iters, i);
            return 1;
        }
    return 0;
}

int main() {
    const int32_t shapes[][2] = {{1, 1}, {3, 1}, {1, 4}, {5, 7}, {37, 19}, {70, 66}, {300, 2}};
    const int32_t iters[] = {1, 5, 8};
    int runs = 0;
    for (const auto& s : shapes)
        for (int32_t it : iters) {
            if (run(s[0], s[1], it)) return 1;
            ++runs;
        }
    printf("denoise sanitize: %d runs ok\n", runs);
    return 0;
}
