// pt_walk_lines_host.cpp — TEST INFRASTRUCTURE.  hc_bvh_check / hc_qbvh_check
// (pt_hostcheck.cpp) draw their lines at random, so no direction of theirs has
// a zero or an f32-subnormal component and rcp_dir's +-1e30 branch is never
// taken.  hc_walk_lines runs the same two checks on the caller's lines
// (tests/rays_any_ref.py: axis directions, d.z = 0, components of 1e-39).
// Built by tests/test_rays_any_host.py into a temporary directory by the
// hostcheck Makefile's pattern rule (tests/hostlib.py).
#include "pt_hostcheck.cpp"

extern "C" {

// For each of the n lines (o[i], d[i]) and every BVH triangle the f64
// reference (eval64) says the line meets at sqd: a walk of the BNode tree with
// box_hit and a walk of the QNode tree with the walks' own child test
// (q_child_dist_s on q_line_ex's parameters), both with the kernels' f32 line
// (o - centre, rcp_dir of the unit direction) and range sqrt(sqd)(1 + 1e-6),
// must reach that triangle's leaf; q_child_dist_s must equal q_child_dist bit
// for bit on every child tested and reject every absent child.
// out: [0] hits checked, [1] leaves the BNode walk missed, [2] leaves the
// QNode walk missed, [3] child tests whose two forms differ, [4] child tests
// compared, [5] absent children let in, [6] lines with a slab parameter
// (1/d, or A, B of a node met) that is not finite, [7] lines with a zero or
// subnormal f32 direction component.
int hc_walk_lines(const pt_scene_desc* d, const double* o, const double* dir, int64_t n, int64_t* out) {
    HostScene H;
    if (!prepare_scene(d, &H).empty()) return -1;
    bind_host(&H);
    const SceneK& K = H.k;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (K.n_bunit == 0 || K.n_qnode == 0) return -3;
    std::vector<int> bleaf(K.n_bunit, -1), qleaf(K.n_bunit, 0);
    for (int i = 0; i < K.n_bnode; ++i) {
        const BNode& B = H.bnode[i];
        if (B.leaf >= 0)
            for (int q = B.leaf >> 3; q < (B.leaf >> 3) + (B.leaf & 7); ++q) bleaf[q] = i;
    }
    for (int q = 0; q < K.n_qnode; ++q)
        for (int c = 0; c < 4; ++c) {
            const int r = H.qnode[q].ref[c];
            if (r <= -2)
                for (int i = 0; i < ((~r) & 7); ++i) qleaf[((~r) >> 3) + i] = r;
        }
    std::vector<char> visited(K.n_bnode);
    std::vector<int> reached;
    for (int64_t r = 0; r < n; ++r) {
        const D3 oo = d3(o[3 * r], o[3 * r + 1], o[3 * r + 2]);
        const D3 dn = unit(d3(dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]));
        const F3 d32 = to_f3(dn);
        const F3 o32 = to_f3(oo - ld3(K.center)), inv = rcp_dir(d32);
        bool odd = !(std::isfinite(inv.x) && std::isfinite(inv.y) && std::isfinite(inv.z));
        if (fabsf(d32.x) < 1.17549435e-38f || fabsf(d32.y) < 1.17549435e-38f || fabsf(d32.z) < 1.17549435e-38f)
            ++out[7];
        for (int q = 0; q < K.n_bunit; ++q) {
            const UnitF& U = H.bunit[q];
            for (int m = 0; m < U.count; ++m) {
                D3 Q; double sqd;
                if (!eval64(H.trid[U.t[m]], oo, dn, &Q, &sqd)) continue;
                const float R = (float)(sqrt(sqd) * (1 + 1e-6));
                ++out[0];
                std::fill(visited.begin(), visited.end(), 0);
                int node = 0;
                while (node >= 0) {
                    const BNode& B = H.bnode[node];
                    const F3 l = {B.lo[0] - o32.x, B.lo[1] - o32.y, B.lo[2] - o32.z};
                    const F3 h = {B.hi[0] - o32.x, B.hi[1] - o32.y, B.hi[2] - o32.z};
                    const bool hit = box_hit(l, h, inv, R);
                    if (hit) visited[node] = 1;
                    node = (hit && B.leaf < 0) ? node + 1 : B.skip;
                }
                if (!visited[bleaf[q]]) ++out[1];
                reached.clear();
                std::vector<int> st{K.qroot};
                while (!st.empty()) {
                    const int nd = st.back();
                    st.pop_back();
                    if (nd <= -2) { reached.push_back(nd); continue; }
                    const QNode& N = H.qnode[nd];
                    const QLine L = q_line_ex(N, o32, inv);
                    const QSlabs SL = q_slabs(N, L);
                    for (int a = 0; a < 3; ++a) odd = odd || !std::isfinite(L.A[a]) || !std::isfinite(L.B[a]);
                    for (int c = 0; c < 4; ++c) {
                        const float es = q_child_dist_s(SL, c, L, R);
                        if (N.ref[c] == kNoRef) {
                            if (q_child_dist_s(SL, c, L, INFINITY) != INFINITY) ++out[5];
                            continue;
                        }
                        const float e = q_child_dist(N, c, L, R);
                        ++out[4];
                        if (memcmp(&e, &es, sizeof e) != 0) ++out[3];
                        if (es < INFINITY) st.push_back(N.ref[c]);
                    }
                }
                if (std::find(reached.begin(), reached.end(), qleaf[q]) == reached.end()) ++out[2];
            }
        }
        if (odd) ++out[6];
    }
    return 0;
}

}  // extern "C"
