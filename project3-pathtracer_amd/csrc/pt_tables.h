// pt_tables.h -- the scene tables configure() (pt_context.hip) hands to the device, built on the host: world triangles, culling
// bounds, light table, boxes, slabs, material planes, motion knots, the hierarchy and the camera-ray span tables.  Host code only:
// nothing here touches the HIP runtime; every function reads its inputs and fills vectors.
#pragma once
#include <stdint.h>

#include <vector>

#include "pt_internal.h"

namespace pt {

struct Aabb { float lo[3], hi[3]; };

// what the tables are built from: the context's scene, camera and options
struct SceneInput {
    const std::vector<pt_static_geom> &geoms;
    const std::vector<pt_static_geom> &geoms_next;   // the geoms at the end of the shutter interval (motion blur), or empty
    const std::vector<pt_material> &mats;
    const std::vector<float> &tri_obj;               // triangles of the MESH geoms, object space: 9 floats each ...
    const std::vector<int> &tri_geom;                //   ... and the geom they belong to
    const pt_camera_data &cam;
    const pt_camera_data *cam_next;                  // the camera at the end of the shutter interval, or nullptr
    float lens_radius;
    int nknots;                                      // motion blur with a shutter time per ray: knot states (0 = off)
    int motion_rotat;
};

struct SceneTables {
    std::vector<float> triw;                    // world triangles, 12 floats each: v0, e1, e2, unit normal
    std::vector<double> reach, tri_reach;       // how far from geom i / triangle t a ray tested against it can start
    std::vector<ptd::Prim> prims;               // geoms, then triangles (at least one record)
    std::vector<LightRec> lights;
    std::vector<int> light_tris;
    std::vector<float> light_cdf;
    std::vector<float> ro_eye;                  // per primitive: inverseTransform * (eye, 1), float4
    std::vector<float> face_n;                  // per primitive: 8 float4 of box-face normals (+ cube-light thresholds)
    std::vector<Aabb> boxes;                    // per primitive: padded world box for hit-or-miss culling
    std::vector<float> box_world, box_eye;      // the same as (lo.xyz, 0)(hi.xyz, 0), world / relative to the eye
    std::vector<float> slab_n;                  // per primitive (n.xyz, d_lo) of a tilted cube's slab (d_hi: box_world[8 i + 7])
    uint32_t slab_mask = 0u;
    std::vector<float> mat_planes;              // ptd::M_PLANES planes of one float per material (at least one material)
    std::vector<float> knots, knot_cam, swept;  // per-ray motion blur: transform rows and camera per knot, swept world boxes
    std::vector<ptd::BvhNode> bvh;              // binary hierarchy (at least one node; nnodes of them real)
    std::vector<float> bvh4;                    // its 4-wide form (at least one record; nnodes4 of them real)
    int nnodes = 0, nnodes4 = 0, wdepth = 0;
    int nbig = 0, big[16] = {};                 // primitives too large to cull, outside the hierarchy
};

SceneTables build_tables(const SceneInput &s);

// pixel-independent camera basis and the tile's pixel mapping (KParams: eye .. focal_distance, W .. pix_offset, w_*, strip_*)
void set_view(KParams &k, const pt_camera_data &cam, const pt_options &o, int W, int row_begin, int npix);
float fov_tan(float degrees);

// camera-ray span tables, if the launch shape `cfg` takes them (KParams: the camera, the tile mapping, the table sizes)
std::vector<uint32_t> span_mask(const KParams &k, const LaunchCfg &cfg, const SceneTables &t);
void span_lists(const KParams &k, const LaunchCfg &cfg, const SceneTables &t, std::vector<uint32_t> &off, std::vector<uint32_t> &lst);

pt_vec3 lerp3(pt_vec3 a, pt_vec3 b, float t);

}  // namespace pt
