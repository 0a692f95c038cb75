// pt_lens_wf_host.cpp — TEST INFRASTRUCTURE.  The thin-lens wavefront state
// machine (pt_wavefront.h wf_slot_step<AA, true>, the text k_wf_shade_lens and
// k_wf_shade_list_lens run) run on the host, in its uniform form (a whole
// frame, `split` slots per pixel) and its list form (one accumulator pass),
// on pt_aa_wf_host.cpp's buffers, loop and finals (wf_render, wf_pass) — a lens run finds what
// an antialiased run left, and the other way round — so the CPU suite can
// check it against the single kernel's lane code (pt_lens_host.cpp
// hc_render_lens) and the oracle's per-sample colours through the lens without
// a GPU.  Built by tests/test_lens_wavefront_host.py into a temporary
// directory by the hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_aa_wf_host.cpp"

extern "C" {

// hc_aa_wf_render through the lens L: the whole frame of p (PT_FLAG_AA in
// p->flags: jittered as well), `split` slots per pixel; sum [H*W][3] f64 in
// image orientation, the pixel's slots reduced in store_pixel's xor order.
int hc_lens_wf_render(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, uint32_t split,
                      int fresh, double* sum, int32_t* steps_out, int32_t* busy, int32_t busy_cap) {
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!L || !open_scene(d, &H, L)) return -1;
    return wf_render(H.k, p, true, (p->flags & PT_FLAG_AA) != 0, split, fresh, sum, steps_out, busy, busy_cap);
}

// hc_aa_wf_pass through the lens L (k_wf_shade_list_lens's step over the
// active list, k_wf_final_list): one pass over list[0..n_list) under the rule,
// `split` slots per entry; S, Q, n read and updated in place.
int hc_lens_wf_pass(const pt_scene_desc* d, const pt_lens* L, const pt_render_params* p, const uint32_t* list,
                    uint32_t n_list, uint32_t min_spp, uint32_t max_spp, uint32_t step_spp, uint32_t split,
                    int fresh, double* accS, double* accQ, uint32_t* accN, int32_t* steps_out, int32_t* busy,
                    int32_t busy_cap) {
    if (!split_ok(split)) return -4;
    HostScene H;
    if (!L || !open_scene(d, &H, L)) return -1;
    return wf_pass(H.k, p, true, (p->flags & PT_FLAG_AA) != 0, list, n_list,
                   AdaptK{0.0, 1.0, min_spp, max_spp, step_spp}, split, fresh, accS, accQ, accN, steps_out, busy,
                   busy_cap);
}

// the C ABI's additive record of this change (tests: its size is pinned)
int hc_launch_info_size() { return (int)sizeof(pt_launch_info); }
int hc_api_version() { return PT_API_VERSION; }

}  // extern "C"
