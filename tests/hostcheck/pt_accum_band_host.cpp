// pt_accum_band_host.cpp — TEST INFRASTRUCTURE.  The band mapping of the
// accumulator's select (pt_path.h BandK, band_make, band_pixel) compiled for
// the host on top of pt_hostcheck.cpp, so the CPU suite can compare it with
// _abi.band_pixels and a direct construction from _abi.band_rows.  Built by
// tests/test_adaptive_bands.py into a temporary directory by the hostcheck
// Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

extern "C" {

// The band's pixel count; with out != NULL also e of each band pixel b, in
// order (at most cap of them).
int64_t hc_band_pixels(int32_t W, int32_t H, int32_t row_begin, int32_t row_end, int32_t row_step,
                       int32_t row_phase, uint32_t* out, int64_t cap) {
    const BandK B = band_make(W, H, row_begin, row_end, row_step, row_phase);
    if ((uint64_t)B.rows * (uint64_t)W != (uint64_t)B.npix) return -1;
    for (uint32_t b = 0; out && b < B.npix && (int64_t)b < cap; ++b) out[b] = band_pixel(B, b);
    return (int64_t)B.npix;
}

}  // extern "C"
