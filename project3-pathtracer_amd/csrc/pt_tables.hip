// pt_tables.hip -- host side: the scene tables configure() uploads (pt_tables.h).  No HIP runtime calls in this unit.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pt_scene.h"
#include "pt_tables.h"

namespace pt {
namespace {

struct v3 { float x, y, z; };
v3 cross3(v3 x, v3 y) { return {x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y}; }
v3 normalize3(v3 v)
{
    float inv = 1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return {v.x * inv, v.y * inv, v.z * inv};
}
float length3(v3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }

// multiplyMV(m, (x, y, z, w)) with the reference's operation order (ref: src/intersections.h:53-59); the w term stays even for
// w = 0 (an infinite or NaN entry of the fourth column shows through, as it does in the reference)
v3 mv(const pt_mat4 &m, float x, float y, float z, float w)
{
    return {(m.x.x * x) + (m.x.y * y) + (m.x.z * z) + (m.x.w * w),
            (m.y.x * x) + (m.y.y * y) + (m.y.z * z) + (m.y.w * w),
            (m.z.x * x) + (m.z.y * y) + (m.z.z * z) + (m.z.w * w)};
}

// the columns of a transform's upper 3x3 in double, their lengths and dot products (every caller judges orthogonality with a
// threshold and a comparison of its own: they differ on NaN)
struct Columns {
    double col[3][3], len[3];
    explicit Columns(const pt_mat4 &m)
    {
        const float *r0 = &m.x.x, *r1 = &m.y.x, *r2 = &m.z.x;
        for (int j = 0; j < 3; ++j) {
            col[j][0] = r0[j]; col[j][1] = r1[j]; col[j][2] = r2[j];
            len[j] = sqrt(col[j][0] * col[j][0] + col[j][1] * col[j][1] + col[j][2] * col[j][2]);
        }
    }
    double dot(int a, int b) const { return col[a][0] * col[b][0] + col[a][1] * col[b][1] + col[a][2] * col[b][2]; }
    bool orthogonal(double tol) const         // (a NaN dot product passes)
    {
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 3; ++b)
                if (fabs(dot(a, b)) > tol * len[a] * len[b]) return false;
        return true;
    }
};

// getRadiuses' half-extents of a transformed unit cube / r = .5 sphere in fp32 (ref: src/intersections.h:120-129)
void half_extents(const pt_mat4 &m, float r[3])
{
    const v3 org = mv(m, 0, 0, 0, 1.0f), ax[3] = {mv(m, .5f, 0, 0, 1.0f), mv(m, 0, .5f, 0, 1.0f), mv(m, 0, 0, .5f, 1.0f)};
    for (int a = 0; a < 3; ++a) {
        const float dx = ax[a].x - org.x, dy = ax[a].y - org.y, dz = ax[a].z - org.z;
        r[a] = sqrtf(dx * dx + dy * dy + dz * dz);
    }
}

// a cube light's side areas and total area with the sampler's fp32 operations (ref: src/intersections.h:140-170)
struct CubeSides { float side1, side2, side3, total; };
CubeSides cube_sides(const float r[3])
{
    const float side1 = r[0] * r[1] * 4.0f, side2 = r[2] * r[1] * 4.0f, side3 = r[0] * r[2] * 4.0f;
    return {side1, side2, side3, 2.0f * (side1 + side2 + side3)};
}

// What the REFERENCE'S sphere test hits is not the sphere.  Its radicand, b*b - (ro.ro - 0.25) with b = ro.rd, is formed from fp32
// products of object-space coordinates (ref: src/intersections.h:81-117; the outer subtraction alone is in double): for a ray that
// starts R object units away both terms are ~ R^2 and carry ~ 16 ulp-halves of it, so the test reports a hit whenever the ray passes
// within sqrt(0.25 + E) of the centre, E <= 20 eps R^2 + 64 eps (s_max / s_min) R (the second term: rounding of the transformed
// direction, seen from R away), eps = 2^-24 -- and its hit point lies within that radius too.  A sphere of radius 0.11 met from 15 world
// units away is 1 % larger than it is; one of radius 0.01 across a room of 100 is hit by rays that pass several radii away.  The oracle
// renders exactly that, so every culling bound of a sphere is taken around the INFLATED sphere: this returns sqrt(1 + 4 E) for rays
// that start at most D world units from the centre (scene_reach() bounds D by the scene).  Cubes: the slab distances err by a few ulps
// of themselves, i.e. by ~ 1e-7 D in world units whatever the scale: an absolute pad.
double sphere_noise_factor(const pt_static_geom &g, double D)
{
    if (!(D > 0.0)) return 1.0;
    const Columns m(g.transform);
    const double(*col)[3] = m.col;
    const double *len = m.len;
    double F2 = 0.0;
    for (int j = 0; j < 3; ++j) F2 += len[j] * len[j];
    double smin, smax;
    if (m.orthogonal(1e-4)) {
        smin = std::min(len[0], std::min(len[1], len[2])) * (1.0 - 2e-4);
        smax = std::max(len[0], std::max(len[1], len[2])) * (1.0 + 2e-4);
    } else {                                  // singular values: s_max <= ||M||_F, s_min = |det| / (s_1 s_2) >= 2 |det| / ||M||_F^2
        const double det = col[0][0] * (col[1][1] * col[2][2] - col[1][2] * col[2][1]) - col[1][0] * (col[0][1] * col[2][2] - col[0][2] * col[2][1]) +
                           col[2][0] * (col[0][1] * col[1][2] - col[0][2] * col[1][1]);
        smax = sqrt(F2);
        smin = 2.0 * fabs(det) / F2;
    }
    const double eps = 5.9604644775390625e-8, FMAX = 1e6;
    if (!(smin > 0.0) || !(smax > 0.0)) return FMAX;
    const double R = D / smin + 0.5;
    const double E = 20.0 * eps * R * R + 64.0 * eps * (smax / smin) * R;
    const double f = sqrt(1.0 + 4.0 * E);
    return f < FMAX ? f : FMAX;                 // (a NaN compares false: FMAX)
}

// Padded world-space box of one primitive: |x_a - c_a| <= 0.5 * sum_i |M[a][i]| for the unit cube and
// <= 0.5 * sqrt(sum_i M[a][i]^2) for the r = .5 sphere (M = rows 0..2 of the transform); +1 % and +1e-3 absorb the
// fp32 rounding of the traversal's slab test and the 1e-4 back-off of getPointOnRay.  D: how far from the primitive's centre a ray
// tested against it can start (0: not known yet) -- sphere_noise_factor above.
Aabb prim_bounds(const pt_static_geom &g, double rel, double abs_pad, double D)
{
    const float *rows[3] = {&g.transform.x.x, &g.transform.y.x, &g.transform.z.x};
    Aabb b;
    const double noise = (g.type == PT_SPHERE) ? sphere_noise_factor(g, D) : 1.0;
    abs_pad += 2e-6 * D;
    for (int a = 0; a < 3; ++a) {
        const double m0 = rows[a][0], m1 = rows[a][1], m2 = rows[a][2], c = rows[a][3];
        double h = (g.type == PT_SPHERE) ? 0.5 * sqrt(m0 * m0 + m1 * m1 + m2 * m2) * noise : 0.5 * (fabs(m0) + fabs(m1) + fabs(m2));
        h = h * rel + abs_pad + 1e-6 * fabs(c);
        b.lo[a] = (float)(c - h);
        b.hi[a] = (float)(c + h);
    }
    return b;
}

// padded world box of the world triangle w (12 floats: v0, e1, e2, normal; culling only), same padding rule as prim_bounds: + 2e-6 x
// reach for what the reference's test and the kernels' slab tests lose on a ray that starts that far away (a unit triangle seen from
// 1e6 units is fuzzy by ~ 0.1)
Aabb tri_bounds(const float *w, double rel, double abs_pad, double reach)
{
    Aabb b;
    abs_pad += 2e-6 * reach;
    for (int a = 0; a < 3; ++a) {
        const double p0 = w[a], p1 = (double)w[a] + w[3 + a], p2 = (double)w[a] + w[6 + a];
        const double lo = std::min(p0, std::min(p1, p2)), hi = std::max(p0, std::max(p1, p2));
        const double cc = 0.5 * (lo + hi), h = 0.5 * (hi - lo) * rel + abs_pad + 1e-6 * fabs(cc);
        b.lo[a] = (float)(cc - h);
        b.hi[a] = (float)(cc + h);
    }
    return b;
}

// ---- culling hierarchy over the primitives (host build; the kernels only read it) -------------------------
void build_bvh(const std::vector<Aabb> &boxes, std::vector<int> &idx, size_t lo, size_t hi, std::vector<ptd::BvhNode> &nodes)
{
    const size_t me = nodes.size();
    nodes.push_back(ptd::BvhNode());
    Aabb u = boxes[(size_t)idx[lo]];
    float cmin[3], cmax[3];
    for (int a = 0; a < 3; ++a) cmin[a] = cmax[a] = 0.5f * (u.lo[a] + u.hi[a]);
    for (size_t k = lo + 1; k < hi; ++k) {
        const Aabb &b = boxes[(size_t)idx[k]];
        for (int a = 0; a < 3; ++a) {
            if (b.lo[a] < u.lo[a]) u.lo[a] = b.lo[a];
            if (b.hi[a] > u.hi[a]) u.hi[a] = b.hi[a];
            const float cc = 0.5f * (b.lo[a] + b.hi[a]);
            if (cc < cmin[a]) cmin[a] = cc;
            if (cc > cmax[a]) cmax[a] = cc;
        }
    }
    if (hi - lo == 1) {
        nodes[me].prim = idx[lo];          // the caller ORs the primitive type into bit 30
    } else {
        // surface-area heuristic, full sweep: for every axis sort by centroid and take the split that minimises
        // area(left)*count(left) + area(right)*count(right)  (the hierarchy only culls, so any split is correct)
        const size_t n = hi - lo;
        auto half_area = [](const Aabb &b) {
            const double dx = (double)b.hi[0] - b.lo[0], dy = (double)b.hi[1] - b.lo[1], dz = (double)b.hi[2] - b.lo[2];
            return dx * dy + dy * dz + dz * dx;
        };
        auto grow = [](Aabb &u2, const Aabb &b) {
            for (int a = 0; a < 3; ++a) {
                if (b.lo[a] < u2.lo[a]) u2.lo[a] = b.lo[a];
                if (b.hi[a] > u2.hi[a]) u2.hi[a] = b.hi[a];
            }
        };
        double best_cost = 1e300;
        int best_axis = -1;
        size_t best_left = n / 2;
        auto by_centroid = [&](int axis) {
            return [&boxes, axis](int x, int y) {
                return boxes[(size_t)x].lo[axis] + boxes[(size_t)x].hi[axis] < boxes[(size_t)y].lo[axis] + boxes[(size_t)y].hi[axis];
            };
        };
        if (n <= 4096) {
            // full sweep; only (axis, split position) of the best split are kept during it -- the winning order is rebuilt
            // by one more sort afterwards (stable_sort of the same input: the same order)
            std::vector<int> order(n);
            std::vector<double> right_area(n);
            for (int axis = 0; axis < 3; ++axis) {
                if (!(cmax[axis] > cmin[axis])) continue;
                std::copy(idx.begin() + (long)lo, idx.begin() + (long)hi, order.begin());
                std::stable_sort(order.begin(), order.end(), by_centroid(axis));
                Aabb acc = boxes[(size_t)order[n - 1]];
                for (size_t k = n - 1; k >= 1; --k) {                 // right_area[k] = area of order[k..n)
                    grow(acc, boxes[(size_t)order[k]]);
                    right_area[k] = half_area(acc);
                }
                acc = boxes[(size_t)order[0]];
                for (size_t k = 1; k < n; ++k) {                      // split: left = order[0..k), right = order[k..n)
                    grow(acc, boxes[(size_t)order[k - 1]]);
                    const double cost = half_area(acc) * (double)k + right_area[k] * (double)(n - k);
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_left = k; }
                }
            }
            if (best_axis >= 0) std::stable_sort(idx.begin() + (long)lo, idx.begin() + (long)hi, by_centroid(best_axis));
        } else {
            // large nodes (triangle meshes): binned surface-area heuristic, 32 centroid bins per axis, O(n) per node
            constexpr int NB = 32;
            int best_bin = -1;
            for (int axis = 0; axis < 3; ++axis) {
                if (!(cmax[axis] > cmin[axis])) continue;
                Aabb bb[NB];
                size_t cnt[NB] = {0};
                const double scale = (double)NB / ((double)cmax[axis] - (double)cmin[axis]);
                auto bin_of = [&](int x) {
                    const double cc = 0.5 * ((double)boxes[(size_t)x].lo[axis] + (double)boxes[(size_t)x].hi[axis]);
                    int b = (int)((cc - (double)cmin[axis]) * scale);
                    return b < 0 ? 0 : (b >= NB ? NB - 1 : b);
                };
                for (size_t k = lo; k < hi; ++k) {
                    const int b = bin_of(idx[k]);
                    if (cnt[b]++ == 0) bb[b] = boxes[(size_t)idx[k]]; else grow(bb[b], boxes[(size_t)idx[k]]);
                }
                double ra[NB];
                size_t rc[NB];
                Aabb acc{};
                size_t c2 = 0;
                for (int b = NB - 1; b >= 1; --b) {                  // right side = bins [b, NB)
                    if (cnt[b]) { if (c2 == 0) acc = bb[b]; else grow(acc, bb[b]); c2 += cnt[b]; }
                    ra[b] = c2 ? half_area(acc) : 0.0;
                    rc[b] = c2;
                }
                c2 = 0;
                for (int b = 1; b < NB; ++b) {                       // left side = bins [0, b)
                    if (cnt[b - 1]) { if (c2 == 0) acc = bb[b - 1]; else grow(acc, bb[b - 1]); c2 += cnt[b - 1]; }
                    if (c2 == 0 || rc[b] == 0) continue;
                    const double cost = half_area(acc) * (double)c2 + ra[b] * (double)rc[b];
                    if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; best_left = c2; }
                }
            }
            if (best_axis >= 0) {
                const int axis = best_axis;
                const double scale = (double)NB / ((double)cmax[axis] - (double)cmin[axis]);
                std::stable_partition(idx.begin() + (long)lo, idx.begin() + (long)hi, [&](int x) {
                    const double cc = 0.5 * ((double)boxes[(size_t)x].lo[axis] + (double)boxes[(size_t)x].hi[axis]);
                    int b = (int)((cc - (double)cmin[axis]) * scale);
                    b = b < 0 ? 0 : (b >= NB ? NB - 1 : b);
                    return b < best_bin;
                });
            }
        }
        const size_t mid = lo + best_left;
        nodes[me].prim = -1;
        build_bvh(boxes, idx, lo, mid, nodes);
        build_bvh(boxes, idx, mid, hi, nodes);
    }
    for (int a = 0; a < 3; ++a) { nodes[me].lo[a] = u.lo[a]; nodes[me].hi[a] = u.hi[a]; }
    nodes[me].skip = (uint32_t)nodes.size();          // first node after this subtree
}


// 4-wide hierarchy for geom_path 7, collapsed from the binary one (depth-first, skip links: the left child of internal
// node i is i + 1, the right child is nodes[i + 1].skip): a wide node takes the two children of a binary node and keeps
// replacing the child with the largest box by that child's own two children until it has four (or only leaves are left).
// Record = ptd::W4_FLOATS floats: per axis the four children's lo planes then their hi planes (x: [0..8), y: [8..16),
// z: [16..24)), then four child words (bit 31 leaf, bit 30 cube, bit 29 triangle, bits 9..28 node / primitive index; the low
// nine bits stay free for the owner lane and the three direction signs of a traversal entry).  An empty child has lo = +3e38, hi = -3e38: no ray passes.
int build_wide4(const std::vector<ptd::BvhNode> &bin, const std::vector<int> &ptype, int b, int depth,
                std::vector<float> &out, int &maxdepth)
{
    auto is_leaf = [&](int i) { return bin[(size_t)i].prim >= 0; };
    auto area = [&](int i) {
        const ptd::BvhNode &n = bin[(size_t)i];
        const double dx = (double)n.hi[0] - n.lo[0], dy = (double)n.hi[1] - n.lo[1], dz = (double)n.hi[2] - n.lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    std::vector<int> kids;
    if (is_leaf(b)) kids.push_back(b);                    // a one-primitive hierarchy: the root is that leaf
    else { kids.push_back(b + 1); kids.push_back((int)bin[(size_t)b + 1].skip); }
    while (kids.size() < 4) {
        int best = -1;
        for (size_t k = 0; k < kids.size(); ++k)
            if (!is_leaf(kids[k]) && (best < 0 || area(kids[k]) > area(kids[(size_t)best]))) best = (int)k;
        if (best < 0) break;
        const int n = kids[(size_t)best];
        kids[(size_t)best] = n + 1;
        kids.push_back((int)bin[(size_t)n + 1].skip);
    }
    const int me = (int)(out.size() / ptd::W4_FLOATS);
    out.resize(out.size() + ptd::W4_FLOATS, 0.0f);
    if (depth > maxdepth) maxdepth = depth;
    for (int c = 0; c < 4; ++c) {
        uint32_t word = 0u;
        float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
        if (c < (int)kids.size()) {
            const ptd::BvhNode &n = bin[(size_t)kids[(size_t)c]];
            for (int a = 0; a < 3; ++a) { lo[a] = n.lo[a]; hi[a] = n.hi[a]; }
            if (n.prim >= 0) {
                const uint32_t prim = (uint32_t)n.prim & 0x3FFFFFFFu;
                word = 0x80000000u | (ptype[prim] == PT_CUBE ? 0x40000000u : 0u) | (ptype[prim] == 3 ? 0x20000000u : 0u) | (prim << 9);
            } else {
                word = (uint32_t)build_wide4(bin, ptype, kids[(size_t)c], depth + 1, out, maxdepth) << 9;
            }
        }
        float *rec = out.data() + (size_t)me * ptd::W4_FLOATS;       // (re-fetched: the recursion grows the vector)
        for (int a = 0; a < 3; ++a) { rec[8 * a + c] = lo[a]; rec[8 * a + 4 + c] = hi[a]; }
        memcpy(&rec[24 + c], &word, 4);
    }
    return me;
}

// triangles of the MESH geoms in world space (12 floats each: v0, e1, e2, unit normal), evaluated with multiplyMV's
// operation order; they are primitives of their own behind the geoms: index = number of geoms + triangle number
std::vector<float> world_triangles(const SceneInput &s)
{
    const size_t nT = s.tri_geom.size();
    std::vector<float> triw(nT * 12);
    for (size_t t = 0; t < nT; ++t) {
        const pt_mat4 &m = s.geoms[(size_t)s.tri_geom[t]].transform;
        v3 w[3];
        for (int j = 0; j < 3; ++j) {
            const float *p = &s.tri_obj[9 * t + 3 * (size_t)j];
            w[j] = mv(m, p[0], p[1], p[2], 1.0f);
        }
        float *o12 = &triw[12 * t];
        const v3 e1 = {w[1].x - w[0].x, w[1].y - w[0].y, w[1].z - w[0].z}, e2 = {w[2].x - w[0].x, w[2].y - w[0].y, w[2].z - w[0].z};
        const v3 cr = cross3(e1, e2);
        const float l2 = cr.x * cr.x + cr.y * cr.y + cr.z * cr.z;
        const v3 n = (l2 > 0.0f) ? normalize3(cr) : v3{0, 0, 0};
        o12[0] = w[0].x; o12[1] = w[0].y; o12[2] = w[0].z;
        o12[3] = e1.x; o12[4] = e1.y; o12[5] = e1.z;
        o12[6] = e2.x; o12[7] = e2.y; o12[8] = e2.z;
        o12[9] = n.x; o12[10] = n.y; o12[11] = n.z;
    }
    return triw;
}

// reach[i]: how far from the centre of geom i a ray that is tested against it can start -- the eye (the lens around it) or a point
// of (the padded bounds of) any primitive, at either end of a motion.  The bounds of spheres depend on it (sphere_noise_factor), so
// this is a fixed point: the inflation is ~ 1e-3 of the reach for ordinary shapes and the iteration settles at once; a scene where it
// does not (spheres squeezed by factors of hundreds) gets the largest reach the factor knows, and culls nothing of them.
// tri_reach[t]: the same for triangle t, from the sphere around every point a ray can start from that the fixed point ends with
// (the triangles' own bounds take no reach inside the iteration).
void scene_reach(const SceneInput &s, const std::vector<float> &triw, std::vector<double> &reach, std::vector<double> &tri_reach)
{
    const size_t nGeoms = s.geoms.size(), nT = s.tri_geom.size();
    reach.assign(nGeoms, 0.0);
    tri_reach.assign(nT, 0.0);
    double scene_c0[3] = {0, 0, 0}, scene_rs = 0.0;
    bool settled = false;
    for (int pass = 0; pass < 8 && !settled; ++pass) {
        double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        bool first = true;
        auto grow = [&](const double *l, const double *h) {
            for (int a = 0; a < 3; ++a) {
                if (first || l[a] < lo[a]) lo[a] = l[a];
                if (first || h[a] > hi[a]) hi[a] = h[a];
            }
            first = false;
        };
        auto grow_box = [&](const Aabb &b) {
            const double l[3] = {b.lo[0], b.lo[1], b.lo[2]}, h[3] = {b.hi[0], b.hi[1], b.hi[2]};
            grow(l, h);
        };
        auto grow_eye = [&](const pt_camera_data &cam) {
            const double r = s.lens_radius > 0.0f ? (double)s.lens_radius * 1.001 : 0.0;
            const double l[3] = {cam.position.x - r, cam.position.y - r, cam.position.z - r};
            const double h[3] = {cam.position.x + r, cam.position.y + r, cam.position.z + r};
            grow(l, h);
        };
        grow_eye(s.cam);
        if (s.cam_next) grow_eye(*s.cam_next);
        for (size_t i = 0; i < nGeoms; ++i) {
            if (s.geoms[i].type == PT_MESH) continue;
            grow_box(prim_bounds(s.geoms[i], 1.01, 1e-3, reach[i]));
            if (!s.geoms_next.empty()) grow_box(prim_bounds(s.geoms_next[i], 1.01, 1e-3, reach[i]));
        }
        for (size_t t = 0; t < nT; ++t) grow_box(tri_bounds(&triw[12 * t], 1.01, 1e-3, 0.0));
        const double c0[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
        const double rs = 0.5 * sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
        scene_c0[0] = c0[0]; scene_c0[1] = c0[1]; scene_c0[2] = c0[2];
        scene_rs = rs * 1.002;             // (the triangles' own pads, 2e-6 of it, are inside the 0.2 %)
        settled = true;
        for (size_t i = 0; i < nGeoms; ++i) {
            auto dist = [&](const pt_static_geom &g) {
                const double dx = g.transform.x.w - c0[0], dy = g.transform.y.w - c0[1], dz = g.transform.z.w - c0[2];
                return sqrt(dx * dx + dy * dy + dz * dz);
            };
            double d = dist(s.geoms[i]);
            if (!s.geoms_next.empty()) d = std::max(d, dist(s.geoms_next[i]));
            d += rs;
            if (!(d <= reach[i])) { settled = false; reach[i] = d * 1.002; }          // (a NaN never settles)
        }
    }
    if (!settled) { for (size_t i = 0; i < nGeoms; ++i) reach[i] = 1e9; scene_rs = 1e9; }
    if (getenv("PT_NO_NOISE_PAD")) { for (size_t i = 0; i < nGeoms; ++i) reach[i] = 0.0; return; }      // (ablation: rounds 1-3's bounds)
    for (size_t t = 0; t < nT; ++t) {
        const float *w = &triw[12 * t];
        const double cx = w[0] + ((double)w[3] + w[6]) / 3.0, cy = w[1] + ((double)w[4] + w[7]) / 3.0, cz = w[2] + ((double)w[5] + w[8]) / 3.0;
        const double dx = cx - scene_c0[0], dy = cy - scene_c0[1], dz = cz - scene_c0[2];
        tri_reach[t] = (sqrt(dx * dx + dy * dy + dz * dz) + scene_rs) * 1.002;
    }
}

// device records of the primitives: geoms, then triangles (at least one record)
std::vector<ptd::Prim> prim_records(const SceneInput &s, const SceneTables &t)
{
    const size_t nGeoms = s.geoms.size(), nT = s.tri_geom.size(), nP = nGeoms + nT;
    std::vector<ptd::Prim> prims(nP ? nP : 1);
    memset(prims.data(), 0, prims.size() * sizeof(ptd::Prim));
    for (size_t i = 0; i < nGeoms; ++i) {
        const pt_static_geom &g = s.geoms[i];
        ptd::Prim &p = prims[i];
        p.type = (uint32_t)g.type;
        p.material = (uint32_t)g.materialid;
        memcpy(p.inv, &g.inverseTransform, 12 * sizeof(float));
        memcpy(p.fwd, &g.transform, 12 * sizeof(float));
        // multiplyMV(transform, (0,0,0,1)) with the reference's operation order (ref: src/intersections.h:53-59,111)
        const pt_mat4 &m = g.transform;
        const v3 centre = mv(m, 0.0f, 0.0f, 0.0f, 1.0f);
        p.cx = centre.x; p.cy = centre.y; p.cz = centre.z;
        // padded bounding sphere: every point of the unit cube / r=.5 sphere lies within half the sum of the
        // transform's column lengths of the centre; +2 % and +1e-3 absorb fp32 rounding of the cull test
        const Columns cm(m);
        const double *len = cm.len;
        double sum = 0.0, sumsq = 0.0, maxlen = 0.0;
        for (int col = 0; col < 3; ++col) {
            sum += len[col]; sumsq += len[col] * len[col];
            if (len[col] > maxlen) maxlen = len[col];
        }
        double rad;                                   // (T*R*S transforms have orthogonal columns)
        if (cm.orthogonal(1e-4)) rad = (g.type == PT_SPHERE) ? 0.5 * maxlen : 0.5 * sqrt(sumsq);   // r*s_max / half diagonal
        else rad = (g.type == PT_SPHERE) ? 0.5 * sqrt(sumsq) : 0.5 * sum;                  // Frobenius / triangle bound
        if (g.type == PT_SPHERE) rad *= sphere_noise_factor(g, t.reach[i]);                // (what the reference's test hits)
        // (+ what the reference's inverseTransform * origin and the cull's own c - o lose far from the world origin)
        rad = rad * 1.02 + 1e-3 + 2e-6 * t.reach[i] + 4e-6 * (fabs((double)p.cx) + fabs((double)p.cy) + fabs((double)p.cz));
        p.bound_r2 = (float)(rad * rad);
        // self_r2: may a ray that leaves this primitive on its OUTSIDE skip it at its next bounce (resident paths)?  Mathematically a
        // ray that starts outside a convex primitive and moves away from it cannot meet it again; the kernels may only rely on
        // that where the REFERENCE'S ARITHMETIC agrees for every such ray (the oracle tests the primitive all the same):
        //  (i)  the shading normal must be the surface normal -- a uniformly scaled sphere (the reference's sphere normal is the
        //       direction from the centre, which an ellipsoid's is not: a ray sampled about it can dive back into an ellipsoid) or a
        //       cube under a transform with orthogonal columns;
        //  (ii) the new origin, hit point + 0.0002 * normal, must really lie outside.  A cube's slab distances are accurate to a few
        //       ulps of the ray's length (error along the face axis ~ 3e-7 * distance in WORLD units, whatever the scale): with the
        //       scene within 128 units that is <= 1e-4 of margin against the 2e-4 bias.  A SPHERE's quadratic is not: b*b - c cancels
        //       for a ray that comes from far away relative to the sphere's size (fp32 error ~ (distance / scale)^2 * 6e-8 object
        //       units), and the reported point can lie inside the sphere by more than the bias -- the path then bounces on inside
        //       (cloud256: a sphere of radius 0.11 met from 12.5 units away; the oracle renders exactly that).  So for spheres the
        //       kernels check the hit point itself: skipping needs |p - c| > r - 0.0002 + margin, i.e. an origin at least `margin`
        //       outside, margin = 2e-5 + 1e-5 * scale + rounding of the check (coordinates up to `coord`);
        //  (iii) moderate sizes: the object-space offset of the bias, 0.0002 / scale, must stay far above fp32 noise (scale <= 64).
        // The bounds-checking build runs the exact test on every skipped pair and reports a hit.
        const bool tight = cm.orthogonal(1e-6);   // (the 1e-4 above only sizes a culling sphere)
        double minlen = len[0];
        for (int col = 1; col < 3; ++col) if (len[col] < minlen) minlen = len[col];
        const bool uniform = maxlen - minlen <= 1e-6 * maxlen;
        const double coord = sqrt((double)p.cx * p.cx + (double)p.cy * p.cy + (double)p.cz * p.cz) + rad;       // (largest coordinate of its surface)
        const bool sane = maxlen <= 64.0 && minlen > 0.0 && coord <= 128.0;      // (a NaN fails every compare)
        p.self_r2 = 0.0f;
        if (tight && sane && g.type == PT_CUBE) p.self_r2 = 1.0f;
        if (tight && sane && g.type == PT_SPHERE && uniform) {
            const double r = 0.5 * maxlen, margin = 2e-5 + 1e-5 * maxlen + 8.0 * coord * 6e-8;
            const double rc = r - 0.0002 + margin;
            if (margin < 1.5e-4 && rc > 0.0) p.self_r2 = (float)(rc * rc * (1.0 + 1e-6));
        }
        if (getenv("PT_NO_SELF_SKIP")) p.self_r2 = 0.0f;      // (ablation switch)
    }
    for (size_t tr = 0; tr < nT; ++tr) {
        ptd::Prim &p = prims[nGeoms + tr];
        const float *w = &t.triw[12 * tr];
        p.type = 3u;
        p.material = (uint32_t)s.geoms[(size_t)s.tri_geom[tr]].materialid;
        for (int q = 0; q < 9; ++q) p.inv[q] = w[q];
        p.fwd[0] = w[9]; p.fwd[1] = w[10]; p.fwd[2] = w[11];
        const double cx = w[0] + (w[3] + w[6]) / 3.0, cy = w[1] + (w[4] + w[7]) / 3.0, cz = w[2] + (w[5] + w[8]) / 3.0;
        double r2 = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double px = w[0] + (j == 1 ? w[3] : (j == 2 ? w[6] : 0.0)) - cx, py = w[1] + (j == 1 ? w[4] : (j == 2 ? w[7] : 0.0)) - cy,
                         pz = w[2] + (j == 1 ? w[5] : (j == 2 ? w[8] : 0.0)) - cz;
            r2 = std::max(r2, px * px + py * py + pz * pz);
        }
        const double rad = sqrt(r2) * 1.02 + 1e-3 + 2e-6 * t.tri_reach[tr] + 4e-6 * (fabs(cx) + fabs(cy) + fabs(cz));
        p.cx = (float)cx; p.cy = (float)cy; p.cz = (float)cz;
        p.bound_r2 = (float)(rad * rad);
    }
    return prims;
}

// direct lighting: the light table -- emissive geoms in list order (at most 16 entries).  A sphere / cube is an
// entry with its surface area from getRadiuses' half-extents (ref: src/intersections.h:120-129) in fp32 with the
// sampler's own operation order; an emissive MESH geom is ONE entry made of its triangles of positive area
// (area-weighted pick by the running fp32 sum of 0.5 |e1 x e2|, then a uniform point).  Prim::area > 0 marks the
// primitives the table covers: only those are left to the explicit sampling when a path hits them by chance.
void light_table(const SceneInput &s, SceneTables &t)
{
    const size_t nGeoms = s.geoms.size(), nT = s.tri_geom.size();
    for (size_t i = 0; i < nGeoms && t.lights.size() < 16; ++i) {
        const pt_static_geom &g = s.geoms[i];
        if (!(s.mats[(size_t)g.materialid].emittance > 0.0f)) continue;
        if (g.type == PT_MESH) {
            float acc = 0.0f;
            const size_t first = t.light_tris.size();
            for (size_t tr = 0; tr < nT; ++tr) {
                if (s.tri_geom[tr] != (int)i) continue;
                const float *w = &t.triw[12 * tr];
                const float a = 0.5f * length3(cross3(v3{w[3], w[4], w[5]}, v3{w[6], w[7], w[8]}));
                if (!(a > 0.0f)) continue;
                acc = acc + a;
                t.light_tris.push_back((int)tr);
                t.light_cdf.push_back(acc);
                t.prims[nGeoms + tr].area = a;
            }
            if (t.light_tris.size() == first) continue;          // no surface: not a light
            t.lights.push_back(LightRec{(int)i, (int)first, (int)(t.light_tris.size() - first), acc});
            continue;
        }
        float r[3];
        half_extents(g.transform, r);
        const float area = g.type == PT_CUBE ? cube_sides(r).total : 4.18879020478639098f * ((r[0] * r[1] + r[0] * r[2]) + r[1] * r[2]);
        t.prims[i].area = area;
        t.lights.push_back(LightRec{(int)i, 0, 0, area});
    }
}

// camera rays all start at the eye: multiplyMV(inverseTransform, (eye,1)) once per primitive, with the
// reference's operation order (ref: src/intersections.h:53-59,85)
std::vector<float> eye_origins(const SceneInput &s, size_t nrec)
{
    const size_t nGeoms = s.geoms.size(), nT = s.tri_geom.size();
    const float ex = s.cam.position.x, ey = s.cam.position.y, ez = s.cam.position.z;
    std::vector<float> ro(nrec * 4, 0.0f);
    for (size_t i = 0; i < nGeoms; ++i) {
        const v3 o = mv(s.geoms[i].inverseTransform, ex, ey, ez, 1.0f);
        ro[4 * i + 0] = o.x; ro[4 * i + 1] = o.y; ro[4 * i + 2] = o.z;
    }
    for (size_t t = 0; t < nT; ++t) {
        ro[4 * (nGeoms + t) + 0] = ex; ro[4 * (nGeoms + t) + 1] = ey; ro[4 * (nGeoms + t) + 2] = ez;
    }
    return ro;
}

// The world normal of a box face depends on (primitive, face) only: normalize(multiplyMV(transform, (+-axis, 0)))
// evaluated here once with the kernels' operation order (boxNormal in pt_device.h), looked up per hit.
// Cube lights: the sampler's face-choice thresholds (ref: src/intersections.h:140-170, same fp32 operations),
// parked in the table's unused entries 3 (t1..t4) and 7 (t5).
std::vector<float> face_table(const SceneInput &s, size_t nrec)
{
    std::vector<float> fnorm(nrec * 32, 0.0f);
    for (size_t i = 0; i < s.geoms.size(); ++i) {
        const pt_mat4 &m = s.geoms[i].transform;
        float *f = &fnorm[i * 32];
        for (int face = 0; face < 8; ++face) {
            const int axis = face & 3;
            if (axis == 3) continue;
            const float sgn = (face & 4) ? -1.0f : 1.0f;
            const float nx = axis == 0 ? sgn : 0.0f, ny = axis == 1 ? sgn : 0.0f, nz = axis == 2 ? sgn : 0.0f;
            const v3 n = normalize3(mv(m, nx, ny, nz, 0.0f));
            f[face * 4 + 0] = n.x; f[face * 4 + 1] = n.y; f[face * 4 + 2] = n.z;
        }
        if (s.geoms[i].type != PT_CUBE) continue;
        float r[3];
        half_extents(m, r);
        const CubeSides cs = cube_sides(r);
        const float side1 = cs.side1, side2 = cs.side2, side3 = cs.side3, totalarea = cs.total;
        f[12 + 0] = side1 / totalarea;
        f[12 + 1] = (side1 * 2) / totalarea;
        f[12 + 2] = ((side1 * 2) + (side2)) / totalarea;
        f[12 + 3] = ((side1 * 2) + (side2 * 2)) / totalarea;
        f[28 + 0] = ((side1 * 2) + (side2 * 2) + (side3)) / totalarea;
    }
    return fnorm;
}

// hit-or-miss culling boxes (no distance pruning): the padding just has to cover fp32 rounding (1e-6 of the coordinates), and a
// tight one keeps a ray that leaves a wall (0.0002 above it) outside that wall's box.  As the kernels read them: world boxes
// (pre-test of the pair queue), boxes relative to the eye (a wave of camera rays covers a small solid angle and skips the
// primitives none of its rays can reach) and the slabs of tilted cubes.
void box_tables(const SceneInput &s, SceneTables &t)
{
    const size_t nGeoms = s.geoms.size(), nP = nGeoms + s.tri_geom.size(), nrec = t.prims.size();
    t.boxes.resize(nP);
    for (size_t i = 0; i < nP; ++i)
        t.boxes[i] = i < nGeoms ? prim_bounds(s.geoms[i], 1.005, 1e-4, t.reach[i])
                                : tri_bounds(&t.triw[12 * (i - nGeoms)], 1.005, 1e-4, t.tri_reach[i - nGeoms]);
    t.box_eye.assign(nrec * 8, 0.0f);
    t.box_world.assign(nrec * 8, 0.0f);
    t.slab_n.assign(nrec * 4, 0.0f);
    float *bw = t.box_world.data(), *be = t.box_eye.data(), *slab_n = t.slab_n.data();
    for (size_t i = 0; i < nP; ++i) {
        const Aabb &b = t.boxes[i];
        for (int a = 0; a < 3; ++a) { bw[8 * i + (size_t)a] = b.lo[a]; bw[8 * i + 4 + (size_t)a] = b.hi[a]; }
        // a TILTED cube fills little of its world box (the bundled scene's walls, with ROTAT read as radians: 10 x 0.01 x 10 slabs at
        // arbitrary angles, whose boxes fill the room): the pre-test also clips the ray against the slab between the two faces of the
        // cube's THINNEST axis, planes n.x = d_lo / d_hi (n in the record's LDS pad, d_lo beside it, d_hi in the far entry's w).
        // Padded like the box (0.5 % + 1e-4 + what the reference's slab arithmetic errs by, 2e-6 x reach, + the rounding of n.o).
        if (i < nGeoms && i < 32 && s.geoms[i].type == PT_CUBE && !getenv("PT_NO_SLAB")) {
            const pt_mat4 &m = s.geoms[i].transform;
            const Columns cm(m);
            const double(*col)[3] = cm.col;
            const double *len = cm.len;
            bool orth = len[0] > 0.0 && len[1] > 0.0 && len[2] > 0.0;
            for (int a = 0; a < 3 && orth; ++a)
                for (int b2 = a + 1; b2 < 3; ++b2)
                    if (!(fabs(cm.dot(a, b2)) <= 1e-5 * len[a] * len[b2])) orth = false;
            const double vbox = ((double)b.hi[0] - b.lo[0]) * ((double)b.hi[1] - b.lo[1]) * ((double)b.hi[2] - b.lo[2]);
            const int ta = len[0] <= len[1] ? (len[0] <= len[2] ? 0 : 2) : (len[1] <= len[2] ? 1 : 2);
            // (worth its dozen and a half instructions per ray and trip only where the slab is a small part of the box: 0.25 below)
            const double hx = 0.5 * ((double)b.hi[0] - b.lo[0]), hy = 0.5 * ((double)b.hi[1] - b.lo[1]), hz = 0.5 * ((double)b.hi[2] - b.lo[2]);
            if (orth && std::isfinite(vbox) && vbox > 0.0) {
                const double n[3] = {col[ta][0] / len[ta], col[ta][1] / len[ta], col[ta][2] / len[ta]};
                const double cc[3] = {m.x.w, m.y.w, m.z.w};
                const double nc = n[0] * cc[0] + n[1] * cc[1] + n[2] * cc[2];
                const double coord = fabs(cc[0]) + fabs(cc[1]) + fabs(cc[2]) + hx + hy + hz;      // |n.o| of any origin that matters is below this + reach
                const double half = 0.5 * len[ta] * 1.005 + 1e-4 + 2e-6 * t.reach[i] + 4e-7 * (coord + t.reach[i]);
                // the box's extent along n: the slab only helps where it is much thinner than that
                const double ext = fabs(n[0]) * hx + fabs(n[1]) * hy + fabs(n[2]) * hz;
                if (half < 0.25 * ext) {
                    slab_n[4 * i + 0] = (float)n[0]; slab_n[4 * i + 1] = (float)n[1]; slab_n[4 * i + 2] = (float)n[2];
                    // (n rounded to fp32 tilts the planes by <= 1e-7 rad: <= 1e-7 x the cube's size across its faces, inside the pad)
                    slab_n[4 * i + 3] = (float)(nc - half);
                    bw[8 * i + 7] = (float)(nc + half);
                    t.slab_mask |= 1u << i;
                }
            }
        }
        const double e[3] = {s.cam.position.x, s.cam.position.y, s.cam.position.z};
        for (int a = 0; a < 3; ++a) {
            const double lo = (double)b.lo[a] - e[a], hi = (double)b.hi[a] - e[a];
            const double pad = 1e-6 * (fabs(lo) + fabs(hi) + fabs(e[a])) + 1e-6;      // fp32 rounding of the subtraction
            be[8 * i + (size_t)a] = (float)(lo - pad);
            be[8 * i + 4 + (size_t)a] = (float)(hi + pad);
        }
        be[8 * i + 7] = bw[8 * i + 7];                  // (the slab's planes stay in world space: the kernel forms n.o for camera rays too)
    }
}

std::vector<float> material_planes(const std::vector<pt_material> &mats)
{
    const size_t nM = mats.size();
    std::vector<float> planes((nM ? nM : 1) * ptd::M_PLANES, 0.0f);
    for (size_t i = 0; i < nM; ++i) {
        const pt_material &m = mats[i];
        planes[ptd::M_CR * nM + i] = m.color.x; planes[ptd::M_CG * nM + i] = m.color.y; planes[ptd::M_CB * nM + i] = m.color.z;
        planes[ptd::M_SR * nM + i] = m.specularColor.x; planes[ptd::M_SG * nM + i] = m.specularColor.y;
        planes[ptd::M_SB * nM + i] = m.specularColor.z;
        planes[ptd::M_REFL * nM + i] = m.hasReflective; planes[ptd::M_REFR * nM + i] = m.hasRefractive;
        planes[ptd::M_IOR * nM + i] = m.indexOfRefraction; planes[ptd::M_EMIT * nM + i] = m.emittance;
        planes[ptd::M_AR * nM + i] = m.absorptionCoefficient.x; planes[ptd::M_AG * nM + i] = m.absorptionCoefficient.y;
        planes[ptd::M_AB * nM + i] = m.absorptionCoefficient.z;
        planes[ptd::M_SCAT * nM + i] = m.hasScatter; planes[ptd::M_RSCT * nM + i] = m.reducedScatterCoefficient;
    }
    return planes;
}

// motion blur with a shutter time per ray: knot states at shutter times j / slices, built as the slices are (TRS
// interpolated component-wise, matrices rebuilt by the loader's buildTransformationMatrix); the kernels interpolate the
// transform's rows and the camera vectors entry-wise between the two knots around a ray's time and invert the result.
// The primitives' padded world boxes SWEPT over the shutter interval (pair path pre-test): a point of the primitive at a
// time between two knots is a convex combination of its images at the knots (the rows are interpolated entry-wise),
// so the box around the knots' boxes holds it.
void motion_knots(const SceneInput &s, SceneTables &t)
{
    const size_t nGeoms = s.geoms.size();
    const int nk = s.nknots;
    t.knots.assign((size_t)nk * nGeoms * 12, 0.0f);
    t.knot_cam.assign((size_t)nk * 12, 0.0f);
    t.swept.assign(nGeoms * 8, 0.0f);
    float *swept = t.swept.data();
    for (int j = 0; j < nk; ++j) {
        const float tm = (float)j / (float)(nk - 1);
        for (size_t i = 0; i < nGeoms; ++i) {
            const pt_static_geom &a = s.geoms[i], &b = s.geoms_next[i];
            pt_mat4 inv;
            const pt_mat4 fwd = ptamd::buildTransformationMatrix(lerp3(a.translation, b.translation, tm), lerp3(a.rotation, b.rotation, tm),
                                                                 lerp3(a.scale, b.scale, tm), s.motion_rotat, &inv);
            memcpy(&t.knots[((size_t)j * nGeoms + i) * 12], &fwd, 12 * sizeof(float));
            pt_static_geom gk = a;
            gk.transform = fwd;
            const Aabb bk = prim_bounds(gk, 1.005, 1e-4, t.reach[i]);
            for (int ax = 0; ax < 3; ++ax) {
                if (j == 0 || bk.lo[ax] < swept[8 * i + (size_t)ax]) swept[8 * i + (size_t)ax] = bk.lo[ax];
                if (j == 0 || bk.hi[ax] > swept[8 * i + 4 + (size_t)ax]) swept[8 * i + 4 + (size_t)ax] = bk.hi[ax];
            }
        }
        const pt_camera_data &ca = s.cam, *cb = s.cam_next;
        const pt_vec3 pos = cb ? lerp3(ca.position, cb->position, tm) : ca.position;
        const pt_vec3 view = cb ? lerp3(ca.view, cb->view, tm) : ca.view;
        const pt_vec3 up = cb ? lerp3(ca.up, cb->up, tm) : ca.up;
        float *cd = &t.knot_cam[(size_t)j * 12];
        cd[0] = pos.x; cd[1] = pos.y; cd[2] = pos.z;
        cd[4] = view.x; cd[5] = view.y; cd[6] = view.z;
        cd[8] = up.x; cd[9] = up.y; cd[10] = up.z;
    }
}

// culling hierarchy (used by geom_path 4 / large scenes) over the culling boxes, binary and 4-wide; MESH primitives have no
// geometry and stay out, primitives spanning > 40 % of the scene go to the always-tested list
void hierarchy(const SceneInput &s, SceneTables &t)
{
    const size_t nGeoms = s.geoms.size(), nP = t.boxes.size();
    const std::vector<Aabb> &boxes = t.boxes;
    std::vector<int> ptype(nP, 3);                           // primitive type by expanded index (3 = triangle)
    for (size_t i = 0; i < nGeoms; ++i) ptype[i] = s.geoms[i].type;
    std::vector<int> idx;
    float slo[3] = {0, 0, 0}, shi[3] = {0, 0, 0};
    bool first_box = true;
    for (size_t i = 0; i < nP; ++i) {
        if (ptype[i] == PT_MESH) continue;
        for (int a = 0; a < 3; ++a) {
            if (first_box || boxes[i].lo[a] < slo[a]) slo[a] = boxes[i].lo[a];
            if (first_box || boxes[i].hi[a] > shi[a]) shi[a] = boxes[i].hi[a];
        }
        first_box = false;
    }
    float sext = 0.0f;
    for (int a = 0; a < 3; ++a) if (shi[a] - slo[a] > sext) sext = shi[a] - slo[a];
    for (size_t i = 0; i < nP; ++i) {
        if (ptype[i] == PT_MESH) continue;
        float ext = 0.0f;
        for (int a = 0; a < 3; ++a) if (boxes[i].hi[a] - boxes[i].lo[a] > ext) ext = boxes[i].hi[a] - boxes[i].lo[a];
        // a primitive spanning > 40 % of the scene goes to the always-tested list (at most 16 of them)
        if (ext > 0.4f * sext && t.nbig < 16 && nP > 16) t.big[t.nbig++] = (int)i;
        else idx.push_back((int)i);
    }
    std::vector<ptd::BvhNode> &nodes = t.bvh;
    if (!idx.empty()) build_bvh(boxes, idx, 0, idx.size(), nodes);
    for (auto &nd : nodes)
        if (nd.prim >= 0) nd.prim |= (ptype[(size_t)nd.prim] == PT_CUBE ? 1 : 0) << 30;
    t.nnodes = (int)nodes.size();
    if (!nodes.empty()) build_wide4(nodes, ptype, 0, 1, t.bvh4, t.wdepth);
    t.nnodes4 = (int)(t.bvh4.size() / ptd::W4_FLOATS);
    if (t.bvh4.empty()) t.bvh4.resize(ptd::W4_FLOATS, 0.0f);
    if (nodes.empty()) nodes.push_back(ptd::BvhNode());
}

// Camera rays: which primitives can the 64 pixels of a bounce-0 chunk see at all?  A primitive is dropped for a span of
// 64 tile-local pixels when its padded box lies wholly outside one of the four side planes of the span's pixel frustum
// (grown by a pixel on every side; a span that runs over a row end takes the whole rows) or wholly behind the eye.
// Conservative: that only ever drops (ray, primitive) pairs whose box pre-test would fail in every lane -- the
// bounds-checking build runs those tests anyway and reports any that passes.  Needs rays that start at the eye (no
// lens); the lists also need chunks that are spans (npix % 64 == 0), the table copes with chunks across spans.
struct Frustum { double nrm[4][3], cc[3], lcc; bool planes_ok, narrow; };

// visit(span, its frustum) for spans 0 .. nspan - 1 of 64 tile-local pixels
template <class F>
void for_each_span(const KParams &k, int nspan, F visit)
{
    const int W = k.W, npix = k.npix;
    const double ex = k.eye[0], ey = k.eye[1], ez = k.eye[2];
    const double eye3[3] = {ex, ey, ez};
    const double vw[3] = {(double)k.M[0] - ex, (double)k.M[1] - ey, (double)k.M[2] - ez};
    auto gpix = [&](uint32_t pl) -> uint32_t {
        if (k.strip_span == 0u) return pl + k.pix_offset;
        const uint32_t j = pl / k.strip_span;
        return pl + k.strip_span * (j * (k.strip_world - 1u) + k.strip_rank);
    };
    auto dirOf = [&](double sx, double sy, double *o3) {
        for (int a = 0; a < 3; ++a) o3[a] = vw[a] + (1.0 - 2.0 * sx) * (double)k.H[a] + (1.0 - 2.0 * sy) * (double)k.V[a];
    };
    // The reference forms the point on the image plane in fp32 WORLD coordinates, (M + a H) + b V with M = eye + view, and only then
    // subtracts the eye: far from the world origin the ray directions are quantised to the ulp of the eye's coordinates (an eye at
    // 3e6 sees a 0.25-unit grid through a 1-unit view vector) and leave the ideal pixel frustum by far more than a pixel.  Each
    // component of P - eye errs by <= ~ 3 ulp of the largest coordinate involved; in screen units that is a margin of
    // err / (2 |H|) and err / (2 |V|) on top of the pixel the frustum is grown by.  Past a full screen of margin: no culling.
    double sx_margin, sy_margin;
    {
        double big = 0.0, lh = 0.0, lv = 0.0;
        for (int a = 0; a < 3; ++a) {
            big = std::max(big, fabs(eye3[a]) + fabs(vw[a]) + fabs((double)k.H[a]) + fabs((double)k.V[a]));
            lh += (double)k.H[a] * (double)k.H[a]; lv += (double)k.V[a] * (double)k.V[a];
        }
        const double err = 3.0 * 1.1920929e-7 * big * 1.7320508;           // (vector norm of three such components)
        sx_margin = lh > 0.0 ? err / (2.0 * sqrt(lh)) : 1e30;
        sy_margin = lv > 0.0 ? err / (2.0 * sqrt(lv)) : 1e30;
    }
    const bool ray_grid_ok = sx_margin < 1.0 && sy_margin < 1.0;          // (a NaN fails)
    for (int sp = 0; sp < nspan; ++sp) {
        Frustum f;
        const uint32_t pl1 = (uint32_t)sp * 64u + 63u < (uint32_t)npix ? (uint32_t)sp * 64u + 63u : (uint32_t)npix - 1u;
        const uint32_t g0 = gpix((uint32_t)sp * 64u), g1 = gpix(pl1);
        const int y0 = (int)(g0 / (uint32_t)W), y1 = (int)(g1 / (uint32_t)W);
        int xa = (int)(g0 % (uint32_t)W), xb = (int)(g1 % (uint32_t)W);
        if (y0 != y1) { xa = 0; xb = W - 1; }
        const int ya = y0 < y1 ? y0 : y1, yb = y0 < y1 ? y1 : y0;
        const double sx0 = ((double)xa - 1.0) / (double)k.resx - sx_margin, sx1 = ((double)xb + 2.0) / (double)k.resx + sx_margin;
        const double sy0 = ((double)ya - 1.0) / (double)k.resy - sy_margin, sy1 = ((double)yb + 2.0) / (double)k.resy + sy_margin;
        double cn[4][3];
        dirOf(sx0, sy0, cn[0]); dirOf(sx1, sy0, cn[1]); dirOf(sx1, sy1, cn[2]); dirOf(sx0, sy1, cn[3]);
        dirOf(0.5 * (sx0 + sx1), 0.5 * (sy0 + sy1), f.cc);
        f.planes_ok = ray_grid_ok;
        for (int e = 0; e < 4 && f.planes_ok; ++e) {
            const double *a3 = cn[e], *b3 = cn[(e + 1) & 3];
            const double n3[3] = {a3[1] * b3[2] - b3[1] * a3[2], a3[2] * b3[0] - b3[2] * a3[0], a3[0] * b3[1] - b3[0] * a3[1]};
            const double len = sqrt(n3[0] * n3[0] + n3[1] * n3[1] + n3[2] * n3[2]);
            if (!(len > 1e-12)) { f.planes_ok = false; break; }
            const double sg = (n3[0] * f.cc[0] + n3[1] * f.cc[1] + n3[2] * f.cc[2]) > 0.0 ? -1.0 / len : 1.0 / len;    // outward: the centre is inside
            for (int a = 0; a < 3; ++a) f.nrm[e][a] = n3[a] * sg;
        }
        // "behind the eye" only when every corner direction is within 60 degrees of the centre direction
        f.lcc = sqrt(f.cc[0] * f.cc[0] + f.cc[1] * f.cc[1] + f.cc[2] * f.cc[2]);
        f.narrow = f.planes_ok && f.lcc > 1e-12;
        for (int e = 0; e < 4 && f.narrow; ++e) {
            const double l = sqrt(cn[e][0] * cn[e][0] + cn[e][1] * cn[e][1] + cn[e][2] * cn[e][2]);
            if (!((cn[e][0] * f.cc[0] + cn[e][1] * f.cc[1] + cn[e][2] * f.cc[2]) > 0.5 * l * f.lcc)) f.narrow = false;
        }
        visit(sp, f);
    }
}

// box given relative to the eye
bool outside(const Frustum &f, const double *lo, const double *hi)
{
    if (!f.planes_ok) return false;
    double scale = 1.0;
    for (int a = 0; a < 3; ++a) scale += fabs(lo[a]) + fabs(hi[a]);
    for (int e = 0; e < 4; ++e) {
        double vmin = 0.0;                  // the box corner deepest inside this plane
        for (int a = 0; a < 3; ++a) { const double x = f.nrm[e][a] * lo[a], y = f.nrm[e][a] * hi[a]; vmin += x < y ? x : y; }
        if (vmin > 1e-5 * scale) return true;
    }
    if (f.narrow) {
        double vmax = 0.0;
        for (int a = 0; a < 3; ++a) { const double x = f.cc[a] * lo[a], y = f.cc[a] * hi[a]; vmax += x > y ? x : y; }
        if (vmax < -1e-5 * scale * f.lcc) return true;
    }
    return false;
}

bool spans_ok(const KParams &k) { return k.eye_cull && !(k.lens_radius > 0.0f) && k.npix / 64 <= (1 << 21); }    // (host work: <= 2 M spans, a 134 Mpx tile)

// division by d as multiply + shift, exact for every index < 2^bits: s = bits + ceil(log2 d), m = ceil(2^s / d) < 2^(bits + 1),
// and m*d - 2^s < d <= 2^(s - bits)
void div_magic(uint32_t bits, uint32_t d, uint32_t &magic, uint32_t &shift)
{
    uint32_t lg = 0;
    while ((1ull << lg) < (unsigned long long)d) ++lg;
    shift = bits + lg;
    magic = (uint32_t)(((1ull << shift) + (unsigned long long)d - 1ull) / (unsigned long long)d);
}

}  // namespace

SceneTables build_tables(const SceneInput &s)
{
    SceneTables t;
    t.triw = world_triangles(s);
    scene_reach(s, t.triw, t.reach, t.tri_reach);
    t.prims = prim_records(s, t);
    light_table(s, t);
    t.ro_eye = eye_origins(s, t.prims.size());
    t.face_n = face_table(s, t.prims.size());
    box_tables(s, t);
    t.mat_planes = material_planes(s.mats);
    if (s.nknots > 0) motion_knots(s, t);
    hierarchy(s, t);
    return t;
}

float fov_tan(float degrees)
{
    const double PI = 3.1415926535897932384626422832795028841971;
    return (float)tan((double)degrees * (PI / 180.0));
}

void set_view(KParams &k, const pt_camera_data &cam, const pt_options &o, int W, int row_begin, int npix)
{
    // camera basis: pixel-independent part of raycastFromCameraKernel (DESIGN.md "Canonical semantics", camera)
    const v3 eye = {cam.position.x, cam.position.y, cam.position.z};
    const v3 view = {cam.view.x, cam.view.y, cam.view.z};
    const v3 up = {cam.up.x, cam.up.y, cam.up.z};
    const v3 A = normalize3(cross3(view, up));
    const v3 B = normalize3(cross3(A, view));
    const float lenV = length3(view);
    const float hx = lenV * fov_tan(cam.fov.x), vy = lenV * fov_tan(cam.fov.y);
    k.eye[0] = eye.x; k.eye[1] = eye.y; k.eye[2] = eye.z;
    k.M[0] = eye.x + view.x; k.M[1] = eye.y + view.y; k.M[2] = eye.z + view.z;
    k.H[0] = hx * A.x; k.H[1] = hx * A.y; k.H[2] = hx * A.z;
    k.V[0] = vy * B.x; k.V[1] = vy * B.y; k.V[2] = vy * B.z;
    k.resx = cam.resolution.x; k.resy = cam.resolution.y;
    const v3 vn = normalize3(view);
    k.A[0] = A.x; k.A[1] = A.y; k.A[2] = A.z;
    k.B[0] = B.x; k.B[1] = B.y; k.B[2] = B.z;
    k.vn[0] = vn.x; k.vn[1] = vn.y; k.vn[2] = vn.z;
    k.lens_radius = o.lens_radius > 0.0f ? o.lens_radius : 0.0f;
    k.focal_distance = o.focal_distance;

    k.W = W;
    k.row_begin = row_begin;
    k.npix = npix;
    k.pix_offset = (uint32_t)row_begin * (uint32_t)W;
    // division by the frame width as multiply + shift, exact for every index < 2^29 (the frame has < 2^29 pixels)
    div_magic(29u, (uint32_t)W, k.w_magic, k.w_shift);
    if (o.strip_rows > 0) {
        k.strip_rows = (uint32_t)o.strip_rows; k.strip_world = (uint32_t)o.strip_world; k.strip_rank = (uint32_t)o.strip_rank;
        k.strip_span = (uint32_t)W * (uint32_t)o.strip_rows;
        div_magic(28u, k.strip_span, k.strip_magic, k.strip_shift);     // (exact for every tile-local pixel index, < 2^28)
    }
}

// pair path (<= 32 primitives): one word per span, bit g = primitive g stays (KParams::span_mask); empty: no table
std::vector<uint32_t> span_mask(const KParams &k, const LaunchCfg &cfg, const SceneTables &t)
{
    if (!(spans_ok(k) && !cfg.motion && cfg.geom == 4 && k.nG <= 32 && k.ntri == 0)) return {};
    const int nspan = (k.npix + 63) / 64;                  // (the last one may be short)
    std::vector<uint32_t> tab((size_t)nspan, 0u);
    for_each_span(k, nspan, [&](int sp, const Frustum &f) {
        uint32_t m = 0u;
        for (int g = 0; g < k.nG; ++g) {
            const float *bx = &t.box_eye[(size_t)g * 8];
            const double lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[4], bx[5], bx[6]};
            if (!outside(f, lo, hi)) m |= 1u << g;
        }
        tab[(size_t)sp] = m;
    });
    return tab;
}

// batched walks: per span the list of the primitives that stay -- found by walking the hierarchy with the frustum -- which,
// when it is short, replaces the walk for the camera rays (KParams::span_off / span_list); off stays empty: no lists
void span_lists(const KParams &k, const LaunchCfg &cfg, const SceneTables &t, std::vector<uint32_t> &off, std::vector<uint32_t> &lst)
{
    if (!(spans_ok(k) && k.npix % 64 == 0 && (cfg.geom == 6 || cfg.geom == 7) && k.nG <= 65536)) return;
    const int nspan = k.npix / 64;
    const double eye3[3] = {k.eye[0], k.eye[1], k.eye[2]};
    const uint32_t LIST_MAX = 40;                      // longer than this: the walk is the better deal
    off.assign((size_t)nspan * 2, 0u);
    lst.clear();
    lst.reserve((size_t)nspan * 12);
    const std::vector<ptd::BvhNode> &bn = t.bvh;
    std::vector<uint32_t> cand;
    auto relBox = [&](const float *lo, const float *hi, double *rl, double *rh) {
        for (int a = 0; a < 3; ++a) {
            const double l = (double)lo[a] - eye3[a], h = (double)hi[a] - eye3[a];
            const double pad = 1e-6 * (fabs(l) + fabs(h) + fabs(eye3[a])) + 1e-6;
            rl[a] = l - pad; rh[a] = h + pad;
        }
    };
    for_each_span(k, nspan, [&](int sp, const Frustum &f) {
        cand.clear();
        double rl[3], rh[3];
        for (int b = 0; b < k.nbig; ++b) {
            const size_t g = (size_t)k.big[b];
            relBox(t.boxes[g].lo, t.boxes[g].hi, rl, rh);
            if (!outside(f, rl, rh)) cand.push_back((uint32_t)g);
        }
        bool too_many = false;
        for (uint32_t i = 0; i < (uint32_t)k.nnodes && !too_many;) {
            const ptd::BvhNode &nd = bn[i];
            relBox(nd.lo, nd.hi, rl, rh);
            if (outside(f, rl, rh)) { i = nd.skip; continue; }
            if (nd.prim >= 0) {
                cand.push_back((uint32_t)nd.prim & 0x3FFFFFFFu);
                if (cand.size() > LIST_MAX) too_many = true;
            }
            i = i + 1u;
        }
        off[2 * (size_t)sp] = (uint32_t)lst.size();
        if (too_many) off[2 * (size_t)sp + 1] = 0xFFFFFFFFu;
        else { off[2 * (size_t)sp + 1] = (uint32_t)cand.size(); lst.insert(lst.end(), cand.begin(), cand.end()); }
    });
    if (lst.empty()) lst.push_back(0u);
    if (getenv("PT_DEBUG_CLOCK")) {
        size_t walked = 0;
        for (int sp = 0; sp < nspan; ++sp) walked += off[2 * (size_t)sp + 1] == 0xFFFFFFFFu;
        fprintf(stderr, "[ptamd] camera-ray lists: %d spans, %.1f primitives per listed span, %zu spans walk\n", nspan,
                (double)lst.size() / (double)(nspan - (int)walked > 0 ? nspan - (int)walked : 1), walked);
    }
}

// motion blur: component-wise fp32 interpolation a + (b - a) * t of translation / rotation / scale and the camera vectors
static float lerp1(float a, float b, float t) { return a + (b - a) * t; }
pt_vec3 lerp3(pt_vec3 a, pt_vec3 b, float t) { return {lerp1(a.x, b.x, t), lerp1(a.y, b.y, t), lerp1(a.z, b.z, t)}; }

}  // namespace pt
