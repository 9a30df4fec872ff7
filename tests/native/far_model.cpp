// far_model.cpp — the ray queries' box test over the far-ray families (tests/far_rays.py;
// tests/test_far_rays_cpu.py; DESIGN.md §5 "Query slack").  pad_model.cpp's sibling: the same scene file,
// builder tree, root-to-leaf boxes and 27 reciprocal variants (it compiles pad_model.cpp for them, that
// program's main renamed), over the builder's untrimmed boxes, each ray with its own tmin and tmax and
// bestT = the oracle's t.  Per cell of the ray file: the oracle's hits, those the render kernels' test
// (clamp_dir, one origin term per axis, the builder's pad alone) loses, those the queries' test
// (hippt_slab.h query_*, the code rayloop::prepare_query runs) loses, and the slack the cell needs.
//
// usage: far_model SCENE.bin RAYS.bin   (the files tests/test_far_rays_cpu.py writes)
#define main pad_model_render_main  // pad_model.cpp's program: its scene reader, Model and tree walk are shared
#include "pad_model.cpp"
#undef main

namespace {

// The parent's test: box_hit with clamp_dir and one origin term, the ray's own tmin.
bool passes_parent(const std::vector<Box> &path, const float o[3], const float d[3], float tmin, float t) {
    float inv[3][3];
    for (int a = 0; a < 3; ++a) {
        const float r = rcp_rn(slab::clamp_dir(d[a]));
        inv[a][0] = std::nextafterf(r, -INFINITY), inv[a][1] = r, inv[a][2] = std::nextafterf(r, INFINITY);
    }
    for (const Box &b : path)
        for (int v = 0; v < 27; ++v) {
            const float ix = inv[0][v % 3], iy = inv[1][(v / 3) % 3], iz = inv[2][v / 9];
            const bool nx = std::signbit(ix), ny = std::signbit(iy), nz = std::signbit(iz);
            float n;
            if (!slab::box_hit(nx ? b.hi[0] : b.lo[0], nx ? b.lo[0] : b.hi[0], ny ? b.hi[1] : b.lo[1],
                               ny ? b.lo[1] : b.hi[1], nz ? b.hi[2] : b.lo[2], nz ? b.lo[2] : b.hi[2], ix, iy, iz,
                               slab::origin_term(o[0], ix), slab::origin_term(o[1], iy), slab::origin_term(o[2], iz), tmin,
                               t, n))
                return false;
        }
    return true;
}

// The queries' test (hippt_slab.h query_*), the slack a parameter: the kernels' is slab::kQuerySlack.
bool passes_query(const std::vector<Box> &path, const float o[3], const float d[3], float tmin, float t, float M,
                  bool full, float slack) {
    const float dmax = std::fmax(std::fabs(d[0]), std::fmax(std::fabs(d[1]), std::fabs(d[2])));
    const float omax = std::fmax(std::fabs(o[0]), std::fmax(std::fabs(o[1]), std::fabs(o[2])));
    const float reach = omax + M, away = slab::query_away(omax, M);
    const float floor = slab::query_dir_floor(dmax, reach);
    float inv[3][3];
    for (int a = 0; a < 3; ++a) {
        const float r = rcp_rn(slab::query_clamp_dir(d[a], floor));
        inv[a][0] = std::nextafterf(r, -INFINITY), inv[a][1] = r, inv[a][2] = std::nextafterf(r, INFINITY);
    }
    for (int v = 0; v < 27; ++v) {
        const float i3[3] = {inv[0][v % 3], inv[1][(v / 3) % 3], inv[2][v / 9]};
        const float tb = slab::query_far_bound(
            reach, std::fmin(std::fabs(i3[0]), std::fmin(std::fabs(i3[1]), std::fabs(i3[2]))));
        float on[3], of[3];
        for (int a = 0; a < 3; ++a) slab::query_origin_terms(o[a], d[a], i3[a], floor, tb, away, slack, on[a], of[a]);
        if (full && slab::query_all_boxes(dmax, reach))  // (a scene with spheres: rayloop::prepare_query)
            for (int a = 0; a < 3; ++a) on[a] = slab::kAllBoxesNear, of[a] = -slab::kAllBoxesNear;
        const bool nx = std::signbit(i3[0]), ny = std::signbit(i3[1]), nz = std::signbit(i3[2]);
        for (const Box &b : path) {
            float n;
            if (!slab::box_hit_query(nx ? b.hi[0] : b.lo[0], nx ? b.lo[0] : b.hi[0], ny ? b.hi[1] : b.lo[1],
                                     ny ? b.lo[1] : b.hi[1], nz ? b.hi[2] : b.lo[2], nz ? b.lo[2] : b.hi[2], i3[0], i3[1],
                                     i3[2], on[0], on[1], on[2], of[0], of[1], of[2], tmin, t, n))
                return false;
        }
    }
    return true;
}

// The oracle's closest hit of a query's ray: argmin (t, id) over t >= tmin, then t < tmax.
int closest_query(const Model &m, const float *ray, float &tBest) {
    int best = -1;
    tBest = INFINITY;
    for (int i = 0; i < m.in.ntris; ++i) {
        float t;
        if (po_tri_hit(&m.tris[size_t(i)], ray, ray + 4, ray[3], &t) && t < tBest) tBest = t, best = i;
    }
    for (int j = 0; j < m.in.nsph; ++j) {
        const float *q = &m.in.spheres[4 * size_t(j)];
        float t;
        if (po_sphere_t(q, q[3] * q[3], ray, ray + 4, ray[3], &t) && t < tBest) tBest = t, best = m.in.ntris + j;
    }
    return best >= 0 && tBest < ray[7] ? best : -1;
}

// A triangle without area (two corners equal, or all three on a line) in exact arithmetic: the oracle
// can still accept it when its determinant rounds away from zero.
bool zero_area(const float *v) {
    const double e1[3] = {double(v[3]) - v[0], double(v[4]) - v[1], double(v[5]) - v[2]};
    const double e2[3] = {double(v[6]) - v[0], double(v[7]) - v[1], double(v[8]) - v[2]};
    return e1[1] * e2[2] - e1[2] * e2[1] == 0 && e1[2] * e2[0] - e1[0] * e2[2] == 0 && e1[0] * e2[1] - e1[1] * e2[0] == 0;
}

// Per cell of the family file: the oracle's hits, those the parent's test loses, those the queries'
// test loses at kQuerySlack, and the smallest slack (units of 2^-24 of the ray's reach, the origin's
// largest |component| + M, so an absolute requirement that grows with K; powers of two from 1/4;
// 0: none needed beyond the relative clamp) at which every hit of the cell passes.  Hits of triangles
// without area are counted apart.
int run_query_cells(Model &m, const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    struct CellIn {
        int start, stop;
        double K, s;
        char label[32];
    };
    int hdr[2];
    std::vector<CellIn> cells;
    std::vector<float> rays;
    bool ok = std::fread(hdr, sizeof(int), 2, f) == 2 && hdr[0] >= 0 && hdr[1] >= 0;
    if (ok) {
        cells.resize(size_t(hdr[1]));
        rays.resize(size_t(hdr[0]) * 8);
        for (CellIn &c : cells)
            ok = ok && std::fread(&c.start, 4, 1, f) == 1 && std::fread(&c.stop, 4, 1, f) == 1 &&
                 std::fread(&c.K, 8, 1, f) == 1 && std::fread(&c.s, 8, 1, f) == 1 && std::fread(c.label, 32, 1, f) == 1;
        ok = ok && (rays.empty() || std::fread(rays.data(), 4, rays.size(), f) == rays.size());
    }
    std::fclose(f);
    if (!ok) return 2;
    std::printf("query_model pad=%.9g M=%.9g slack_units=%.2f\n", double(m.pad), double(m.M),
                double(slab::kQuerySlack) * 16777216.0);
    for (CellIn &c : cells) {
        c.label[31] = 0;
        if (c.start < 0 || c.stop < c.start || c.stop > hdr[0]) return 2;
        int hits = 0, lostParent = 0, lostQuery = 0, degenerate = 0;
        double need = 0;
        const bool full = m.in.nsph > 0;
        for (int i = c.start; i < c.stop; ++i) {
            const float *r = &rays[size_t(i) * 8];
            float t;
            const int prim = closest_query(m, r, t);
            if (prim < 0) continue;
            ++hits;
            if (prim < m.in.ntris && zero_area(&m.in.verts[9 * size_t(prim)])) {
                ++degenerate;  // its t is rounding noise over rounding noise, no point of the ray: not a box's to keep
                continue;
            }
            const std::vector<Box> &p = m.path[size_t(prim)];
            if (!passes_parent(p, r, r + 4, r[3], t)) ++lostParent;
            if (!passes_query(p, r, r + 4, r[3], t, m.M, full, slab::kQuerySlack)) ++lostQuery;
            if (!passes_query(p, r, r + 4, r[3], t, m.M, full, 0.0f)) {
                double q = 0.25;
                while (q < 1e6 && !passes_query(p, r, r + 4, r[3], t, m.M, full, float(q) * 0x1p-24f)) q *= 2;
                need = std::max(need, q);
            }
        }
        std::printf("cell %s K=%.9g s=%.9g rays=%d hits=%d degenerate=%d lost_parent=%d lost_query=%d need_units=%.2f\n",
                    c.label, c.K, c.s, c.stop - c.start, hits, degenerate, lostParent, lostQuery, need);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    Model m;
    if (!read_scene(argv[1], m.in)) {
        std::fprintf(stderr, "far_model: cannot read %s\n", argv[1]);
        return 2;
    }
    const SceneIn &in = m.in;
    m.tris.resize(size_t(in.ntris));
    for (int i = 0; i < in.ntris; ++i) po_tri_setup(&in.verts[9 * size_t(i)], &m.tris[size_t(i)]);
    // the scene upload's boxes, extent hint and tree, as pad_model.cpp's main builds them
    const int numPrims = in.ntris + in.nsph;
    std::vector<float> boxes(size_t(numPrims) * 6);
    for (int i = 0; i < in.ntris; ++i)
        for (int a = 0; a < 3; ++a) {
            const float *v = &in.verts[9 * size_t(i)];
            boxes[6 * size_t(i) + a] = std::min(v[a], std::min(v[3 + a], v[6 + a]));
            boxes[6 * size_t(i) + 3 + a] = std::max(v[a], std::max(v[3 + a], v[6 + a]));
        }
    for (int j = 0; j < in.nsph; ++j) {
        const float *q = &in.spheres[4 * size_t(j)];
        const float r = std::fabs(q[3]) * (1.0f + 1.0f / 4096.0f);
        for (int a = 0; a < 3; ++a) {
            boxes[6 * size_t(in.ntris + j) + a] = q[a] - r;
            boxes[6 * size_t(in.ntris + j) + 3 + a] = q[a] + r;
        }
    }
    float extent = 0.0f;
    for (int a = 0; a < 3; ++a) extent = std::max(extent, float(std::fabs(in.lookfrom[a])));
    Bvh bvh;
    Bvh4 b4;
    std::string err;
    if (!build_bvh_boxes(boxes.data(), numPrims, extent, bvh, err)) {
        std::fprintf(stderr, "far_model: %s\n", err.c_str());
        return 2;
    }
    m.pad = bvh.pad;
    m.M = m.pad * 65536.0f;
    BvhParams sah;
    sah.collapse = 1;
    collapse_bvh4(bvh, b4, sah);
    m.path.resize(size_t(numPrims));
    std::vector<Box> cur;
    collect_paths(m, bvh, b4, 0, cur);
    const int rc = run_query_cells(m, argv[2]);
    if (rc) std::fprintf(stderr, "far_model: cannot read %s\n", argv[2]);
    return rc;
}
