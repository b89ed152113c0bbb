/*
 * ptrt.h -- C ABI of the MI355X (gfx950) path-tracing back end.
 *
 * This is the drop-in boundary for ONE hot path of Mark-Rindler/PTRT-game-engine:
 * the per-pixel path-tracing render loop behind `Scene::render_to_device`
 * (reference: src/pathtracer/scene/scene.cuh:1028-1209, kernel
 * src/pathtracer/scene/scene_kernels.cuh:122-194).  Every entry point below
 * names the reference interface it replaces.  Signatures are plain C: pointers,
 * sizes, ints.  No HIP, torch or C++ types cross this boundary.
 *
 * All functions returning `int` return PTRT_OK (0) on success or a negative
 * PTRT_E_* code; `ptrt_last_error(ctx)` gives the text.  The library never
 * falls back to a CPU implementation: with no usable HIP device every call that
 * needs one fails with PTRT_E_NO_DEVICE.
 *
 * Conventions shared with the reference:
 *   - HDR / G-buffers are row-major, y = 0 is the TOP of the view
 *     (scene_kernels.cuh:130-136); the RGB8 image is BOTTOM-UP, kernel row y is
 *     written to byte row H-1-y (scene.cuh:2013-2015).
 *   - material index == mesh index (path_logic.cuh:818-820).
 *   - one random stream per pixel, keyed by the GLOBAL pixel index y*W+x
 *     (scene_kernels.cuh:33-34), so a tile of a frame renders bit-identically
 *     to the same rows of the full frame.
 */
#ifndef PTRT_H
#define PTRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTRT_ABI_VERSION 6 /* 6: + ptrt_launch_ms_history, + ptrt_set_instance_transforms / ptrt_refit_tlas / ptrt_read_tlas, + ptrt_reorder_tlas / ptrt_read_tlas_order / ptrt_set_instance_transforms_device, + ptrt_set_instance_poses_device / ptrt_read_instance_transforms, + ptrt_query_radiance / ptrt_camera_rays / ptrt_init_rng_states, + ptrt_query_probes, + ptrt_lds_layout, + ptrt_read_bvh (additions only); 2: ptrt_scene_desc gained env_rgba / env_width / env_height; 3: + ptrt_post_frame, ptrt_update_instances; 4: + ptrt_ring_*, ptrt_farm_* (additions only); 5: ptrt_stats gained shadow_rays_walked (the struct grew: rebuild callers of ptrt_get_stats) */

enum {
    PTRT_OK = 0,
    PTRT_E_INVALID = -1,   /* bad argument / inconsistent scene arrays        */
    PTRT_E_NO_DEVICE = -2, /* no HIP device or device index out of range      */
    PTRT_E_HIP = -3,       /* a HIP runtime call failed                       */
    PTRT_E_NOT_READY = -4, /* render before geometry/materials were uploaded  */
    PTRT_E_NOMEM = -5
};

/* ---- plain-data mirrors of the reference's device structs ---------------- */

typedef struct ptrt_vec3 { float x, y, z; } ptrt_vec3; /* common/vec3.cuh:8 (12 B) */

/* DeviceBVHNode, pathtracer/scene/mesh.cuh:37-43 (40 B).  Inner node: count==0,
 * left/right = child node indices.  Leaf: count>0, start = first slot in the
 * primitive-index array. */
typedef struct ptrt_bvh_node {
    ptrt_vec3 bmin, bmax;
    int32_t left, right, start, count;
} ptrt_bvh_node;

typedef struct ptrt_tri { int32_t v0, v1, v2; } ptrt_tri; /* mesh.cuh:45-47 */

/* Host-side description of one mesh: what DeviceMesh (math/intersection.cuh:90-106)
 * holds, with host pointers.  Matrices are the 16 floats of the reference's
 * mat4 exactly as Transform3D::updateMatrices leaves them
 * (scene/transform.cuh:260-306); the path reads them as ROW-major 3x4
 * (intersection.cuh:258-281). */
typedef struct ptrt_mesh_desc {
    const ptrt_vec3 *verts;
    int32_t vert_count;
    const ptrt_tri *faces;
    int32_t face_count;
    const ptrt_bvh_node *nodes; /* BLAS, pre-order, node 0 = root */
    int32_t node_count;
    const int32_t *prim_indices; /* leaf slots -> face index */
    int32_t prim_count;
    float world[16];
    float inverse[16];
    float normal[16];
    int32_t has_transform; /* scene.cuh:718-721 */
} ptrt_mesh_desc;

/* Light, pathtracer/scene/lights.cuh:14-26 (60 B, same field order). */
enum { PTRT_LIGHT_POINT = 0, PTRT_LIGHT_DIRECTIONAL = 1, PTRT_LIGHT_SPOT = 2 };
typedef struct ptrt_light {
    int32_t type;
    ptrt_vec3 position, direction, color;
    float intensity, range;
    float inner_cone, outer_cone; /* COSINES of the half angles (scene.cuh:1539-1540) */
    float radius;
} ptrt_light;

/* The ray-generation part of Camera (scene/camera.cuh:32-39). */
typedef struct ptrt_camera {
    ptrt_vec3 origin, lower_left_corner, horizontal, vertical, u, v, w;
    float lens_radius;
} ptrt_camera;

/* DeviceMaterials, scene/material_lib.cuh:107-125: struct of 17 arrays, each
 * `count` long (host pointers here). */
typedef struct ptrt_materials {
    const ptrt_vec3 *albedo;
    const ptrt_vec3 *specular;
    const float *metallic;
    const float *roughness;
    const ptrt_vec3 *emission;
    const float *ior;
    const float *transmission;
    const float *transmission_roughness;
    const float *clearcoat;
    const float *clearcoat_roughness;
    const ptrt_vec3 *subsurface_color; /* carried, unused by the path */
    const float *subsurface_radius;    /* carried, unused by the path */
    const float *anisotropy;           /* carried, unused by the path */
    const float *sheen;
    const ptrt_vec3 *sheen_tint;
    const float *iridescence;
    const float *iridescence_thickness;
    int32_t count;
} ptrt_materials;

/* Everything `path_trace_kernel` receives that is not a frame buffer
 * (scene_kernels.cuh:123-129), flattened, host pointers. */
typedef struct ptrt_scene_desc {
    const ptrt_mesh_desc *meshes;
    int32_t mesh_count;
    const ptrt_bvh_node *tlas_nodes;
    int32_t tlas_node_count;
    const int32_t *tlas_mesh_indices;
    int32_t tlas_index_count;
    ptrt_materials materials;
    const ptrt_light *lights;
    int32_t light_count;
    ptrt_camera camera;
    ptrt_vec3 sky_top, sky_bottom;
    int32_t use_sky;
    /* Scene::loadHDRI's equirectangular map (scene.cuh:959-1026): env_width*env_height RGBA
     * floats, row 0 = what stbi_loadf returns first with flip_vertically_on_load(true);
     * NULL = none (`d_env_texture == 0`: the sky is the gradient).  ABI version 2. */
    const float *env_rgba;
    int32_t env_width, env_height;
} ptrt_scene_desc;

/* HitInfo, math/intersection.cuh:108-124, as returned by Scene::traceSingleRay. */
typedef struct ptrt_hit {
    int32_t hit;
    float t;
    ptrt_vec3 point, normal;
    int32_t mesh_index;
    int32_t front_face;
    float u, v;
    int32_t face_index;
    ptrt_vec3 local_point;
} ptrt_hit;

/* One ray's answer from ptrt_query_radiance: what a frame leaves for a pixel in PTRT_BUF_ACCUM, _DEPTH, _NORMAL and
 * _OBJECT_ID, in one 32-byte record. */
typedef struct ptrt_radiance {
    float radiance[3]; /* mean over the samples: what ACCUM holds for a pixel */
    float depth;       /* first hit of sample 0, 1e30f on a miss (DEPTH)      */
    float normal[3];   /* first hit of sample 0, zeros on a miss (NORMAL)     */
    int32_t object_id; /* first hit of sample 0, -1 on a miss (OBJECT_ID)     */
} ptrt_radiance;

/* One light probe's answer from ptrt_query_probes: means over the probe's n_dirs rays, 128 bytes.  (Two reserved words, not
 * one: 27 + 3 values and the padding that makes the record one 128-byte row.) */
typedef struct ptrt_probe {
    float sh[9][3];         /* mean of Y_i(d_k) * L_c(p, k): radiance on the real spherical harmonics of bands 0-2, RGB */
    float mean_distance;    /* mean of dist = min(depth, max_distance); a miss has depth 1e30f                           */
    float mean_distance_sq; /* mean of dist * dist                                                                       */
    float hit_fraction;     /* mean of (object_id >= 0 ? 1.0f : 0.0f)                                                    */
    float reserved[2];      /* 0.0f                                                                                      */
} ptrt_probe;

/* One lightmap texel's answer from ptrt_query_irradiance: means over the texel's n_dirs rays, 32 bytes. */
typedef struct ptrt_irradiance {
    float radiance[3];      /* mean of L_c(t, k); irradiance = pi * this for cosine-distributed directions */
    float mean_distance;    /* mean of dist = min(depth, max_distance); a miss has depth 1e30f              */
    float mean_distance_sq; /* mean of dist * dist                                                          */
    float hit_fraction;     /* mean of (object_id >= 0 ? 1.0f : 0.0f)                                       */
    float reserved[2];      /* 0.0f                                                                         */
} ptrt_irradiance;

/* One lightmap texel's answer from ptrt_query_direct: the analytic lights' direct term over Q = light_count * n_shadow shadow
 * samples, 32 bytes. */
typedef struct ptrt_direct {
    float irradiance[3];      /* sum over q of the unblocked samples' weights, divided by (float)n_shadow */
    float lit_fraction;       /* samples walked and not blocked, divided by (float)Q                      */
    float shadowed_fraction;  /* samples blocked, divided by (float)Q                                     */
    float reserved[3];        /* 0.0f                                                                     */
} ptrt_direct;

/* One lightmap texel's answer from ptrt_query_bounce: the analytic lights' one-bounce term over the texel's n_dirs gather rays
 * and the Q = light_count * n_shadow light samples at each ray's hit, 32 bytes. */
typedef struct ptrt_bounce {
    float radiance[3];        /* mean over k of B(t, k); irradiance = pi * this for cosine-distributed directions */
    float lit_fraction;       /* terms walked and not blocked, over (float)(n_dirs * Q)                            */
    float shadowed_fraction;  /* terms blocked, over (float)(n_dirs * Q)                                           */
    float hit_fraction;       /* mean over k of (the gather ray hit ? 1.0f : 0.0f)                                 */
    float reserved[2];        /* 0.0f                                                                              */
} ptrt_bounce;

/* One texel of a lightmap atlas from ptrt_atlas_texels, 32 bytes. */
typedef struct ptrt_atlas_texel {
    float position[3];  /* world                                                                        */
    int32_t face;       /* mesh-local face index; unspecified where mesh < 0                             */
    float normal[3];    /* world, unit, the FRONT side: the side cross(e1, e2) points to                 */
    int32_t mesh;       /* uploaded mesh index, -1 = no triangle covers this texel's centre              */
} ptrt_atlas_texel;

/* One ray hit's answer from ptrt_atlas_sample / ptrt_query_lightmap: the baked atlas read at the hit, 32 bytes. */
typedef struct ptrt_lightmap_sample {
    float rgb[3];   /* the atlas's colour at the hit: sum of w * texel.rgb over the taps used, divided by `weight`; 0 without a tap */
    float weight;   /* sum of the weights of the taps used (bilinear: <= about 1; nearest: 1 or 0)                                   */
    float x, y;     /* the hit in the atlas, texel units (a texel's centre is (i + 0.5, j + 0.5)); 0 without a chart                */
    int32_t face;   /* mesh-local face of the hit (ptrt_hit.face_index), -1 on a miss                                               */
    int32_t mesh;   /* ptrt_hit.mesh_index, -1 on a miss                                                                            */
} ptrt_lightmap_sample;

/* A regular grid of light probes for ptrt_probe_sample / ptrt_query_probe_light.  HOST memory, passed by pointer and copied
 * into the launch. */
typedef struct ptrt_probe_volume {
    float origin[3];    /* position of probe (0, 0, 0)                                                                             */
    float spacing[3];   /* > 0, finite, per axis                                                                                   */
    int32_t counts[3];  /* nx, ny, nz >= 1; probe (i, j, k) is row i + nx*(j + ny*k) of d_probes: ptrt_amd.probes.probe_grid's order */
} ptrt_probe_volume;

/* One surface point's answer from ptrt_probe_sample / ptrt_query_probe_light: the probe volume's irradiance there, 32 bytes. */
typedef struct ptrt_probe_light {
    float irradiance[3]; /* sum of w * E over the corners used, divided by `weight`; 0 without a corner      */
    float weight;        /* sum of the weights of the corners used                                           */
    int32_t cell;        /* row of the footprint's corner 0, -1: no cell                                     */
    int32_t used;        /* bit c set: corner c contributed                                                  */
    int32_t face, mesh;  /* the hit's, -1 on a miss; -1, -1 from ptrt_probe_sample                           */
} ptrt_probe_light;

/* Per-frame counters of the trace stage (Mrays/s numerator). */
typedef struct ptrt_stats {
    uint64_t extension_rays; /* traceRay calls   (intersection.cuh:526) */
    uint64_t shadow_rays;    /* bvh_any_hit_tlas (intersection.cuh:481) */
    uint64_t paths;          /* pixel-samples started                   */
    /* ABI 5.  shadow_rays counts every light sample the reference path sends a shadow ray for (path_logic.cuh:357);
     * a sample whose value is exactly zero whatever its visibility (outside a spot cone, BSDF zero below the horizon)
     * is counted there but its ray is NOT walked by path_trace_kernel.  shadow_rays_walked excludes those, so
     * extension_rays + shadow_rays_walked = rays actually traced (SURVEY 8(d)'s Mrays/s numerator). */
    uint64_t shadow_rays_walked;
} ptrt_stats;

#define PTRT_BLUE_NOISE_SIZE 64 /* common/bluenoise.cuh: 64 x 64 x 2 floats */
#define PTRT_BLUE_NOISE_FLOATS (PTRT_BLUE_NOISE_SIZE * PTRT_BLUE_NOISE_SIZE * 2)
#define PTRT_DEFAULT_SEED 12345ULL /* scene.cuh:448 */

/* buffer kinds for ptrt_read_buffer / ptrt_device_buffer (tile rows only) */
enum {
    PTRT_BUF_ACCUM = 0,     /* float[rows*W*3]  HDR radiance, Scene::getNoisyColorBuffer (scene.cuh:1722) */
    PTRT_BUF_NORMAL = 1,    /* float[rows*W*3]  first-hit normal, getNormalBuffer (scene.cuh:1723)         */
    PTRT_BUF_DEPTH = 2,     /* float[rows*W]    first-hit t,      getDepthBuffer  (scene.cuh:1724)         */
    PTRT_BUF_OBJECT_ID = 3, /* int32[rows*W]    first-hit mesh index (scene_kernels.cuh:193)               */
    PTRT_BUF_RGB8 = 4,      /* uint8[rows*W*3]  tonemapped tile, bottom-up WITHIN the tile                 */
    PTRT_BUF_RNG = 5,       /* uint32[rows*W*6] generator state {d, v0..v4} per pixel (canonical order)     */
    PTRT_BUF_DENOISED = 6,  /* float[H*W*3]     denoiser output (d_denoised_buffer, scene.cuh:1121); denoiser on */
    PTRT_BUF_MOTION = 7,    /* float[H*W*2]     uv motion vectors, Scene::getMotionVectorBuffer (scene.cuh:1725)  */
    PTRT_BUF_RENDER_ACCUM = 8 /* float[rh*rw*3] the path tracer's colour image at the render size: d_scaled_accum
                                 (scene.cuh:181) after ptrt_set_render_size, else the same memory as ACCUM.  With a
                                 reduced render size NORMAL/DEPTH/OBJECT_ID/DENOISED/MOTION are rw x rh as well
                                 (the d_scaled_* set) and ACCUM holds the up-scaled final HDR image (scene.cuh:1194). */
};

typedef struct ptrt_ctx ptrt_ctx;

/* Scene::Scene(w,h) (scene.cuh:747-832): allocates frame buffers and the per-pixel
 * generator states on HIP device `device`.  The context renders rows
 * [tile_y0, tile_y0+tile_rows) of a full_w x full_h frame (tile_rows <= 0 means
 * the whole frame).  Installs nothing else: blue noise, RNG seed, scene are
 * separate calls. */
int ptrt_create(int full_w, int full_h, int tile_y0, int tile_rows, int device, ptrt_ctx **out);

/* Scene::~Scene (scene.cuh:834-941).  NULL and repeated destroy of a dead handle's
 * slot are tolerated the way the reference tolerates double cudaFree. */
void ptrt_destroy(ptrt_ctx *ctx);

/* The same for a context that owns every `period`-th 8-row strip of the frame, starting with strip `phase`
 * (strip t = rows 8t .. 8t+7): the tile farm's other way of cutting a frame (SURVEY 8(e) "interleaved strips ... to
 * balance sky vs geometry").  Contiguous bands of the showcase frame carry 1.6x the mean number of rays in the worst
 * band (three of eight bands are sky); interleaved, every context samples the whole frame.  The context's buffers
 * hold its strips one after the other (top-down; the RGB8 image bottom-up within them, like a band's);
 * period == 1 is the whole frame.  ABI 4. */
int ptrt_create_interleaved(int full_w, int full_h, int phase, int period, int device, ptrt_ctx **out);

const char *ptrt_last_error(const ptrt_ctx *ctx); /* never NULL */
int ptrt_abi_version(void);

/* initBlueNoise() -> cudaMemcpyToSymbol(d_blue_noise) (common/bluenoise.cuh:189-198).
 * `table` = 64*64*2 floats, [y][x][channel]. */
int ptrt_set_blue_noise(ptrt_ctx *ctx, const float *table);

/* Scene::initRandomStates + init_curand_kernel (scene.cuh:433-456,
 * scene_kernels.cuh:26-35): XORWOW state for every pixel of the tile,
 * seed `seed`, subsequence = global pixel index, offset 0. */
int ptrt_reset_rng(ptrt_ctx *ctx, unsigned long long seed);

/* Mesh::upload + Mesh::uploadBVH + Scene::buildAndUploadTLAS's copies + the
 * DeviceMesh descriptor upload (mesh.cuh:330-346,499-516; scene.cuh:458-594,
 * 684-727).  Host arrays are copied (and re-laid-out for the GPU) before return. */
int ptrt_upload_geometry(ptrt_ctx *ctx, const ptrt_mesh_desc *meshes, int mesh_count,
                         const ptrt_bvh_node *tlas_nodes, int tlas_node_count,
                         const int32_t *tlas_mesh_indices, int tlas_index_count);

/* Instances moved, nothing else changed -- the transform-dirty case of Scene::updateAccelerationStructures
 * (scene.cuh:656-743) and of commitObjectChanges (scene.cuh:1784-1787): takes the new world / inverse /
 * normal matrices and has_transform flags of every mesh and the rebuilt TLAS; vertices, BLASes and triangle
 * packets on the device stay where they are (a full ptrt_upload_geometry re-lays-out every triangle).
 * mesh_count must equal the uploaded one.  Read from each descriptor: world, inverse, normal, has_transform -- nothing
 * else (vertex, face and BVH pointers may be stale or NULL).  The meshes' root boxes on the device, which a ptrt_refit /
 * ptrt_build_bvh may have moved since the upload, are left alone; the world-space first-pass boxes of the instances
 * (scenes with a real TLAS) are recomputed from those DEVICE boxes (one small read-back; the call synchronises). */
int ptrt_update_instances(ptrt_ctx *ctx, const ptrt_mesh_desc *meshes, int mesh_count,
                          const ptrt_bvh_node *tlas_nodes, int tlas_node_count,
                          const int32_t *tlas_mesh_indices, int tlas_index_count);

/* Scene::uploadMaterialSoA (scene.cuh:286-431). */
int ptrt_upload_materials(ptrt_ctx *ctx, const ptrt_materials *mats);

/* the d_lights upload in Scene::updateAccelerationStructures (scene.cuh:636-651). */
int ptrt_upload_lights(ptrt_ctx *ctx, const ptrt_light *lights, int light_count);

/* `Camera cam` kernel argument (scene_kernels.cuh:124), set by Scene::setCamera (scene.cuh:1298). */
int ptrt_set_camera(ptrt_ctx *ctx, const ptrt_camera *cam);

/* Scene::setSkyGradient / disableSky (scene.cuh:1548-1565). */
int ptrt_set_sky(ptrt_ctx *ctx, const ptrt_vec3 *top, const ptrt_vec3 *bottom, int use_sky);

/* Scene::loadHDRI's device side (scene.cuh:976-1022): the equirectangular environment map that
 * sampleSky reads with tex2D<float4>(envMap, u, v) (render_utils.cuh:115-137) -- normalised
 * coordinates, address mode wrap in u / clamp in v, linear filtering.  `rgba`: width*height*4
 * floats (host pointer, copied); NULL frees the map (freeHDRI) and the sky is the gradient
 * again.  MI355X has no texture-filtering path worth a detour for one fetch per escaped ray: the
 * bilinear fetch is restated in the kernel with the CUDA texture unit's documented arithmetic
 * (xB = u*W - 0.5, weights quantised to 8 fractional bits).  SURVEY 8(f) rank 4. */
int ptrt_set_env_map(ptrt_ctx *ctx, const float *rgba, int width, int height);

/* Dynamic geometry, same topology (the `Triangles` path of updatePTScene,
 * src/common/PTRTtransfer.cuh:2249-2270, followed by Scene::commitObjectChanges,
 * scene.cuh:1784).  The reference re-allocates the mesh's device arrays and REBUILDS its BVH on
 * the CPU every frame (mesh.cuh:330-346,403-516); here the new vertex positions of mesh
 * `mesh_index` are copied into the arena (`verts`: vert_count x 3 floats, a DEVICE pointer if
 * verts_on_device != 0) and ptrt_refit() re-derives, on the GPU and on the context's stream,
 * the triangle packets, every leaf and inner box of the dirty meshes (bottom-up over the
 * UNCHANGED tree), the mesh root boxes and the TLAS root box.  No host synchronisation.
 * With a TLAS that has inner nodes (more meshes than one TLAS leaf holds) the TLAS itself is left to the
 * caller: follow with ptrt_refit_tlas(), which refits it on the device over the uploaded topology -- or rebuild it over
 * the moved meshes' boxes, as the reference's commit does, and hand it to ptrt_update_instances (the Scene mirror's
 * refitObjectChanges / rebuildObjectChanges do).  A refitted tree has the boxes a
 * host refit of the same topology gives (min/max are exact), so results stay bit-comparable
 * with the oracle run on those arrays; it is NOT the tree a fresh median-split build would give.
 * Host positions (verts_on_device == 0): the caller's buffer is its own again when the call returns, and the call does NOT
 * wait for the stream's earlier work (the previous frame), so the host prepares frame N + 1 while the GPU renders frame N.
 * Ordinary memory is copied into pinned staging memory of the context and crosses PCIe asynchronously on the stream; memory
 * HIP knows as pinned crosses on a copy stream of the context into device staging (the call waits for that transfer alone)
 * and moves into the arena on the stream. */
int ptrt_update_vertices(ptrt_ctx *ctx, int mesh_index, const float *verts, int vert_count, int verts_on_device);
int ptrt_refit(ptrt_ctx *ctx);

/* GPU BVH (re)build of one mesh -- what Scene::updateAccelerationStructures does on the CPU for
 * every dirty mesh (scene.cuh:656-733: Mesh::buildBVH mesh.cuh:403-492 + upload/uploadBVH
 * mesh.cuh:330-346,494-516), for a mesh whose FACE COUNT is unchanged.
 * The reference builder's tree shape depends only on the face count (n > leafTarget+tol splits
 * into n/2 and n-n/2), so the uploaded topology is kept and the faces are re-assigned to the
 * leaf positions in Morton order of their current centroids (30-bit codes, stable radix sort on
 * the GPU), followed by ptrt_refit().  All on the context's stream, nothing returns to the host.
 * Depth and leaf sizes are the uploaded tree's, so the 24-entry stack bound keeps holding.
 * Needs: every face of the mesh in exactly one leaf position (any tree Mesh::buildBVH makes).
 * Behind a TLAS with inner nodes the mesh's new root box reaches the TLAS with ptrt_refit_tlas() (or a host rebuild
 * handed to ptrt_update_instances), as after ptrt_refit; the build itself never depended on the TLAS' shape.
 * ptrt_read_prim_order returns the resulting `primIndices` (mesh.cuh:57) so a
 * host copy of the tree (and the oracle) can follow.
 *
 * ptrt_read_bvh: synchronises; mesh `mesh_index`'s uploaded nodes (pre-order; left / right / start / count as uploaded) with
 * the boxes the DEVICE holds now, after any ptrt_refit / ptrt_build_bvh -- the counterpart of ptrt_read_tlas for one
 * bottom-level tree, so a test can hold every box to the triangles below it.  A node the upload's walk from node 0 did not
 * reach keeps its uploaded box; an absent child has no node and no box to return.  PTRT_E_INVALID for a mesh index outside the
 * upload or unless node_count is the mesh's uploaded node count.  ABI 6, additions only. */
int ptrt_build_bvh(ptrt_ctx *ctx, int mesh_index);
int ptrt_read_prim_order(ptrt_ctx *ctx, int mesh_index, int32_t *prim_indices_out, int count);
int ptrt_read_bvh(ptrt_ctx *ctx, int mesh_index, ptrt_bvh_node *nodes_out, int node_count);

/* Moving instances and meshes behind ANY TLAS without a host round trip (not in the reference, which rebuilds the TLAS on
 * the CPU: scene.cuh:458-594).  The TLAS topology that was uploaded -- child pairs, leaf ranges, mesh indices -- is kept;
 * its boxes are refitted on the device.  A frame's order: any ptrt_update_vertices / ptrt_refit / ptrt_build_bvh, then any
 * ptrt_set_instance_transforms, then ONE ptrt_refit_tlas.  All three are ABI 6 additions.
 *
 * ptrt_set_instance_transforms: the has_transform bit and the world / inverse / normal rows of meshes [first_mesh,
 * first_mesh + count), the fields ptrt_update_instances reads from a descriptor, from HOST memory that is the caller's again
 * on return (pinned staging of the context; the copy and a scatter kernel run on the stream).  No stream synchronisation,
 * no allocation after the first call, root boxes untouched.  A flag that changes the traversal variant takes effect with
 * the next launch.  PTRT_E_INVALID (nothing enqueued) for a range outside the uploaded meshes, a negative count or NULL.
 *
 * ptrt_set_instance_transforms_device: the same records, ranges and refusals, the records lying in DEVICE memory that is
 * ordered on the context's stream (the convention of ptrt_query_rays and verts_on_device).  One scatter launch reads them in
 * place: no copy, no staging, no synchronisation.  World, inverse and normal matrices remain the caller's to compute.  The
 * context's host copy of these fields lags afterwards and is fetched (a synchronisation) by the next call that needs it -- a
 * material upload; until then the growth factor of the instances' first-pass boxes stays what the host last knew, and an
 * instance it does not cover is tested without that box: slower for that instance, never wrong.
 *
 * ptrt_refit_tlas: one launch on the stream (two beyond 4096 meshes) -- every mesh's world box from the root box the
 * DEVICE holds and its world rows (Transform3D::transformAABB's arithmetic), every TLAS leaf box, the inner levels deepest
 * first, the TLAS root box, and the instances' world-space first-pass boxes (PMODE 3), which a ptrt_refit / ptrt_build_bvh
 * / ptrt_set_instance_transforms had invalidated.  The boxes equal a host refit over the same topology bit for bit.  Works
 * for a single-leaf TLAS too.  A refitted TLAS degrades as instances travel (far-apart members of a leaf, overlapping
 * boxes): ptrt_reorder_tlas in its place gives the meshes a fresh order on the device; ptrt_update_instances with a TLAS
 * rebuilt on the host gives the reference's own tree, at the price of a synchronisation.
 *
 * ptrt_reorder_tlas: called where ptrt_refit_tlas would be, and instead of it.  The TLAS keeps its shape (the reference's
 * builder gives a mesh count one shape whatever the boxes are) and the meshes are re-dealt to its indices in Morton order of
 * their world boxes' centres, ties by mesh index -- an object-median split along the Z-order curve, as ptrt_build_bvh does
 * for the faces of a mesh -- followed by the refit above.  One more launch than ptrt_refit_tlas up to 4096 meshes (a sort in
 * LDS), the radix passes of ptrt_build_bvh beyond.  No synchronisation, no allocation, use_graphs 0 and 1; counted by the
 * read-only option "tlas_reorders".  A single-leaf TLAS has nothing to re-deal: the call is ptrt_refit_tlas there.
 * PTRT_E_INVALID (nothing enqueued) if the uploaded tlas_mesh_indices are not a permutation of 0 .. mesh_count - 1.
 *
 * ptrt_read_tlas_order: synchronises; the TLAS index array the device holds now (the counterpart of ptrt_read_prim_order).
 * PTRT_E_INVALID unless count is the uploaded index count.
 *
 * ptrt_read_tlas: synchronises; the uploaded nodes' left / right / start / count with the boxes the device holds now
 * (the counterpart of ptrt_read_prim_order).  PTRT_E_INVALID unless node_count is the uploaded node count.
 *
 * ptrt_set_instance_poses_device: what the reference keeps per mesh -- Transform3D::position, rotation (Euler radians) and
 * scale, nine floats -- from DEVICE memory ordered on the context's stream; one launch derives the has_transform bit and the
 * world / inverse / normal rows of meshes [first_mesh, first_mesh + count) from them and writes them into the mesh records
 * (flag bit 1, the materials', and the root boxes are kept).  No copy, no staging, no allocation, no synchronisation,
 * use_graphs 0 and 1; follow with ONE ptrt_refit_tlas or ptrt_reorder_tlas.  The arithmetic is the reference's host code
 * operation by operation (Transform3D::updateMatrices, transform.cuh:260-306; mat4::operator* with its typo and
 * mat4::inverse with its identity below |det| 1e-10, mat4.cuh:211-323; the has_transform rule of scene.cuh:718-721, which
 * looks at scale.x only): every product and sum rounded separately in the written order, 1 / det and the square roots
 * correctly rounded, sine and cosine the library's own deterministic ones (not a libm's).  A NaN or an infinity propagates as
 * that arithmetic propagates it.  The context's host copy lags as after ptrt_set_instance_transforms_device.  Ranges and
 * refusals as there, and PTRT_E_INVALID (nothing enqueued) unless d_pose is count * 36 bytes of device memory on the
 * context's device: the kernel follows the pointer.
 *
 * ptrt_read_instance_transforms: synchronises; the has_transform bit (0 or 1) and matrices of meshes [first_mesh, first_mesh
 * + count) as the device's mesh records hold them now: rows 0-2 of world, inverse and normal in floats 0-11 (a normal row's
 * fourth word is 0: the records do not keep it), floats 12-15 are 0 0 0 1.  The records may be handed unchanged to
 * ptrt_set_instance_transforms of another context, which reads only those nine rows.  PTRT_E_INVALID for a range outside the
 * uploaded meshes, a negative count or NULL. */
typedef struct ptrt_instance_xform {
    float world[16], inverse[16], normal[16]; /* as in ptrt_mesh_desc */
    int32_t has_transform;
} ptrt_instance_xform;
int ptrt_set_instance_transforms(ptrt_ctx *ctx, int first_mesh, int count, const ptrt_instance_xform *xf);
int ptrt_set_instance_transforms_device(ptrt_ctx *ctx, int first_mesh, int count, const ptrt_instance_xform *d_xf);
int ptrt_refit_tlas(ptrt_ctx *ctx);
int ptrt_read_tlas(ptrt_ctx *ctx, ptrt_bvh_node *nodes_out, int node_count);
int ptrt_reorder_tlas(ptrt_ctx *ctx);
int ptrt_read_tlas_order(ptrt_ctx *ctx, int32_t *mesh_indices_out, int count);
typedef struct ptrt_instance_pose {
    ptrt_vec3 position, rotation, scale; /* Transform3D's state, 36 B */
} ptrt_instance_pose;
int ptrt_set_instance_poses_device(ptrt_ctx *ctx, int first_mesh, int count, const ptrt_instance_pose *d_pose);
int ptrt_read_instance_transforms(ptrt_ctx *ctx, int first_mesh, int count, ptrt_instance_xform *out);

/* The `Triangles` path of updatePTScene with a CHANGING triangle count (PTRTtransfer.cuh:2204-2385:
 * a new triangle list every frame, e.g. a fluid surface).  For a triangle-soup mesh (face i =
 * vertices 3i,3i+1,3i+2, what Scene::addTriangles makes) uploaded with room for N triangles:
 * copies tri_count <= N triangles (9 floats each; a DEVICE pointer if on_device != 0) and turns the
 * remaining N - tri_count into degenerate copies of the last real vertex -- never hit
 * (|det| < EPSILON, intersection.cuh:229), never enlarging a box.  Follow with ptrt_build_bvh(). */
int ptrt_update_triangles(ptrt_ctx *ctx, int mesh_index, const float *verts9, int tri_count, int on_device);

/* ---- post-process "next" row: motion vectors + spatiotemporal denoiser ----
 * DenoiserSettings of the non-split path (src/pathtracer/rendering/denoiser.cuh:36-73); the
 * defaults are the reference's diffuse_* values. */
typedef struct ptrt_denoiser_settings {
    float tau, min_alpha, max_history, sigma_luminance, sigma_normal, sigma_depth;
    int32_t atrous_iterations;
    float clamp_scale, firefly_threshold;
    float depth_reject_absolute, depth_reject_relative, normal_reject_threshold, sky_depth_threshold;
    float edge_depth_threshold, edge_normal_threshold;
    int32_t use_object_ids, enable_firefly_suppression;
} ptrt_denoiser_settings;
void ptrt_denoiser_default_settings(ptrt_denoiser_settings *out);

/* `new Denoiser(settings)` (denoiser.cuh:808-845; created in Scene::updateScaledBuffers,
 * scene.cuh:1978-1993): allocates history + scratch images, marks the next frame as the first.
 * While enabled, ptrt_render runs motion_vector_kernel (denoiser_kernels.cuh:33) with the matrix
 * given to ptrt_set_prev_view_proj, then Denoiser::denoise (denoiser.cuh:966-1064, non-split
 * path), and tonemaps the DENOISED image (scene.cuh:1103-1127,1204).  Full-frame contexts only
 * (the filters read up to 32 pixels across band borders).  settings == NULL: defaults. */
int ptrt_denoiser_enable(ptrt_ctx *ctx, const ptrt_denoiser_settings *settings);
/* Denoiser::destroy + delete (scene.cuh:1970-1976) */
int ptrt_denoiser_disable(ptrt_ctx *ctx);
/* Scene::prev_view_proj (scene.cuh:113,1208,1282): proj*view of the PREVIOUS frame, 16 floats as
 * mat4 stores them (column-major), consumed by the next ptrt_render's motion-vector pass. */
int ptrt_set_prev_view_proj(ptrt_ctx *ctx, const float *m16);

/* ---- post-process "next" row: bloom + resolution scale ----
 * perfSettings.enableBloom (scene.cuh:1137-1183): bright pass (threshold 1.5, knee 0.5), six
 * levels of 5-tap horizontal blur + 5-tap vertical down-sample, five bilinear up-sample-adds,
 * and the last up-sample-add INTO the frame's HDR image (the noisy colour buffer, or the denoised
 * one when the denoiser runs), before the tonemap.  Same arithmetic and the same mip sizes as
 * the reference's host loop, in 8 launches instead of 19 (pt_post.hip.h).  Needs a full-frame
 * context of at least 64x64 (below that a mip level is empty and the reference reads NULL). */
int ptrt_set_bloom(ptrt_ctx *ctx, int enabled);
/* Scene::updateScaledBuffers (scene.cuh:1913-2000) for perfSettings.resolutionScale: path trace,
 * motion vectors, denoiser and bloom run at render_w x render_h (the d_scaled_* buffers; pixel p
 * of the small frame continues generator state p, as the reference's launch does), then
 * upscale_bilinear_kernel (scene_kernels.cuh:406-441) fills the full-size colour buffer, which is
 * tonemapped.  Changing the size frees the denoiser (re-enable it; the reference re-creates it at
 * the new size) -- the caller also restarts accumulation.  The Scene wrapper computes
 * render_w = max(64, int(W * scale)) like the reference.  Full-frame contexts only. */
int ptrt_set_render_size(ptrt_ctx *ctx, int render_w, int render_h);

/* ---- presentation "next" row: the HIP half of rtgl::* ----
 * The reference presents through a CUDA-mapped GL pixel-buffer object
 * (src/common/glfw_view_interop.hpp:281-332: map_pbo_device_ptr -> render_to_device -> unmap_pbo
 * -> blit_pbo_to_texture -> draw_interop).  MI355X has no GL interop, so the PBO becomes a ring of
 * `slots` device RGB8 frames, each mirrored into PINNED host memory:
 *   ptrt_present_map(slot)      = map_pbo_device_ptr: the device pointer to render into (first waits
 *                                 until the slot's previous download has finished)
 *   ptrt_present_unmap(slot)    = unmap_pbo: enqueues the asynchronous device->host copy of the frame
 *                                 on the context's stream and records the slot's event; does not block
 *   ptrt_present_acquire(slot)  = what blit_pbo_to_texture needs: waits for that event and returns the
 *                                 pinned host pixels (W*H*3, bottom-up) for glTexSubImage2D / a file
 * With slots >= 2 the copy of frame i overlaps the rendering of frame i+1 (the viewer maps slot
 * (i+1)%slots while frame i is in flight).  Full-frame or band contexts alike. */
int ptrt_present_create(ptrt_ctx *ctx, int slots);
int ptrt_present_map(ptrt_ctx *ctx, int slot, void **device_pixels);
int ptrt_present_unmap(ptrt_ctx *ctx, int slot);
int ptrt_present_acquire(ptrt_ctx *ctx, int slot, const unsigned char **host_pixels);
int ptrt_present_destroy(ptrt_ctx *ctx);

/* The same ring WITHOUT a context: what rtgl::init_interop_viewer(V, width, height, title, cudaDevice)
 * (glfw_view_interop.hpp:174-279) creates before any Scene exists -- the GL pixel-buffer object registered with
 * CUDA becomes `slots` device frames of `frame_bytes` on `device`, each mirrored into pinned host memory.
 *   ptrt_ring_map     = cudaGraphicsMapResources + GetMappedPointer (glfw_view_interop.hpp:281-298)
 *   ptrt_ring_unmap   = cudaGraphicsUnmapResources (:300-307): enqueues the device->host copy behind the frame.
 *                       ptrt_render / ptrt_post_frame recognise a ring slot as their out_rgb8 and record the
 *                       slot's event on THEIR stream, so the copy waits for exactly that frame and the call site
 *                       stays `map -> scene.render_to_device(ptr) -> unmap`; a slot written by anything else is
 *                       ordered behind all work submitted to the device's blocking streams (NULL-stream event).
 *   ptrt_ring_acquire = what blit_pbo_to_texture (:309-317) needs: waits for the copy, returns the host pixels.
 * Errors: ptrt_last_error(NULL). */
typedef struct ptrt_ring ptrt_ring;
int ptrt_ring_create(int device, size_t frame_bytes, int slots, ptrt_ring **out);
int ptrt_ring_map(ptrt_ring *ring, int slot, void **device_pixels);
int ptrt_ring_unmap(ptrt_ring *ring, int slot);
int ptrt_ring_acquire(ptrt_ring *ring, int slot, const unsigned char **host_pixels);
void ptrt_ring_destroy(ptrt_ring *ring);

/* convenience: the five uploads above from one flattened description */
int ptrt_upload_scene(ptrt_ctx *ctx, const ptrt_scene_desc *scene);

/* The body of Scene::render_to_device (scene.cuh:1028-1209): path_trace_kernel, then -- for
 * full-frame contexts that enabled them -- motion vectors + denoiser, bloom, up-scale, and the
 * tonemap of the final HDR image (fused into whichever stage produces it).  `frame_index` is the reference's frame_count_ (jitter index frame+s,
 * scene_kernels.cuh:152-157; >= 0 -- a negative one is PTRT_E_INVALID: it would index the jitter table out of bounds).  `out_rgb8`: tile_rows*W*3 bytes, bottom-up within
 * the tile; a DEVICE pointer if out_is_device != 0 (the mapped PBO of
 * glfw_view_interop.hpp:281), else a host buffer (synchronous copy).  NULL skips
 * the copy (the RGB8 image stays readable through PTRT_BUF_RGB8).
 * Asynchronous w.r.t. the host when out_is_device != 0 or out_rgb8 == NULL, like
 * the reference (it returns right after the tonemap launch).  Ordering on the context's stream: see option "pipeline" of
 * ptrt_set_option -- the frame is complete before anything that follows the call on the stream, always.
 * out_is_device == PTRT_OUT_DEVICE_FRAME (ABI 5): out_rgb8 is the WHOLE width*height*3 frame (bottom-up) on the context's
 * device and a band / strip context writes its rows where they belong in it -- several contexts on one device fill one
 * frame without a copy (the tile farm does this for the parts on the presenting device).  Not with the denoiser, bloom or a
 * reduced render size; PTRT_BUF_RGB8 then has nothing to read; a presentation-ring slot used this way is marked by the caller
 * that joins the contexts (ptrt_farm_*), not by ptrt_render. */
#define PTRT_OUT_HOST 0
#define PTRT_OUT_DEVICE 1
#define PTRT_OUT_DEVICE_FRAME 2
int ptrt_render(ptrt_ctx *ctx, int frame_index, int spp, int max_depth, void *out_rgb8,
                int out_is_device);

/* cudaDeviceSynchronize at the call sites that have one (scene.cuh:455,1244). */
int ptrt_sync(ptrt_ctx *ctx);

/* synchronising read-back of one tile buffer into host memory */
int ptrt_read_buffer(ptrt_ctx *ctx, int kind, void *host_dst, size_t dst_bytes);

/* Scene::getNoisyColorBuffer/getNormalBuffer/getDepthBuffer (scene.cuh:1722-1725):
 * raw device pointer of a tile buffer (NULL on error).  PTRT_BUF_RNG is not
 * exposed this way (its device layout is private). */
void *ptrt_device_buffer(ptrt_ctx *ctx, int kind);

/* write generator states back in canonical order (tests / checkpointing) */
int ptrt_write_rng(ptrt_ctx *ctx, const uint32_t *states, size_t bytes);

/* Scene::traceSingleRay -> trace_single_ray_kernel (scene.cuh:1367-1391,
 * scene_kernels.cuh:38-49); batched: n rays, origins/directions as n*3 floats in HOST memory.
 * Stages them through device memory it allocates, runs the PTRT_QUERY_CLOSEST query of
 * ptrt_query_rays and synchronises. */
int ptrt_trace_rays(ptrt_ctx *ctx, const float *origins, const float *directions, int n,
                    ptrt_hit *out_hits);

/* Batched ray queries on DEVICE memory (ABI 6, addition only; no counterpart in the reference).
 *   PTRT_QUERY_CLOSEST   out = ptrt_hit[n]: per ray the record ptrt_trace_rays returns (traceRay + the HitInfo fields of
 *                        traceSingleRay); `tmax` must be NULL.
 *   PTRT_QUERY_OCCLUDED  out = int32_t[n]: 1 if bvh_any_hit_tlas(ray, tmax[i]) (intersection.cuh:481-524) finds a hit, else 0
 *                        -- the reference's shadow query: meshes with transmission > 0.5 never occlude, the traversal
 *                        stacks' limits and dropped pushes are the reference's.  `tmax` (n floats) is required.
 * `origins` and `directions` are n*3 floats.  All four pointers must be device memory of the context's device, each
 * allocation large enough for n rays.  The call is enqueued on the context's stream (ptrt_set_stream: the caller's) and
 * returns without synchronising; it allocates and copies nothing.  It runs behind everything earlier on that stream --
 * every earlier ptrt_render of the context (pipelined and split frames are joined onto the stream), geometry uploads,
 * vertex updates, refits, rebuilds, instance updates -- and later frames are ordered behind it, as behind
 * ptrt_render_wireframe.  It touches no generator state, accumulation, G-buffer, RGB8 image, counter of ptrt_get_stats
 * or timing history.  The traversal is the path tracer's for the scene and options (ptrt_get_option "query_pmode":
 * 0 one ray per lane, 1..3 the pair walks; options pair_trace / force_geom).  Band and interleaved contexts answer
 * for the whole scene.  PTRT_E_INVALID for a bad kind, n < 0, a NULL pointer, tmax given for CLOSEST or missing for
 * OCCLUDED, or memory that is not the context's device memory; PTRT_E_NOT_READY before geometry is uploaded; n == 0
 * returns PTRT_OK and launches nothing. */
#define PTRT_QUERY_CLOSEST 0  /* out: ptrt_hit[n]  */
#define PTRT_QUERY_OCCLUDED 1 /* out: int32_t[n]   */
int ptrt_query_rays(ptrt_ctx *ctx, int kind, const float *origins, const float *directions, const float *tmax, int n,
                    void *out);

/* Path-traced radiance for caller-supplied rays on DEVICE memory (ABI 6, addition only; no counterpart in the reference,
 * whose path tracer starts at its own camera).  Per ray i: for s < samples, tracePath(ray i, state i, max_depth)
 * (path_logic.cuh:782-899) with the same ray each time, each sample soft-clamped as path_trace_kernel clamps it
 * (scene_kernels.cuh:170), added in order to a sum that starts at zero, the sum divided by (float)samples; depth, normal and
 * object_id are the first hit of sample 0 (scene_kernels.cuh:179-193).  Fed a pinhole frame's own primary rays
 * (ptrt_camera_rays) and the generator states that frame started from, the records are that frame's ACCUM, DEPTH, NORMAL and
 * OBJECT_ID and the states those the frame leaves, bit for bit: past the primary ray tracePath reads nothing of the pixel.
 * `origins` and `directions` are n*3 floats as for ptrt_query_rays; `rng_states` is n*6 uint32 in the canonical order
 * {d, v0..v4} of PTRT_BUF_RNG / ptrt_write_rng (ptrt_init_rng_states makes fresh ones), read and written back IN PLACE, so a
 * later call continues each ray's stream; `out` is n records.  All four pointers must be device memory of the context's
 * device, each allocation large enough for n rays.  Ordering and side effects are those of ptrt_query_rays: enqueued on the
 * context's stream with no allocation, copy or synchronisation, behind earlier frames, uploads, refits and instance
 * updates; later frames are ordered behind it; it touches none of the context's generator states, accumulation, G-buffers,
 * RGB8 image, ptrt_get_stats counters or timing history.  The traversal is the path tracer's for the scene and options
 * (reported by ptrt_get_option "query_pmode"), the materials the simple or the full set as a frame would choose.  Sky,
 * environment map, lights and materials are the context's current ones; the camera plays no part.  Band and interleaved
 * contexts answer for the whole scene.  PTRT_E_INVALID (nothing enqueued) for n < 0, a NULL pointer, memory that is not the
 * context's device memory, or samples / max_depth outside 1..32767 (ptrt_render's range); PTRT_E_NOT_READY before
 * geometry and materials are uploaded (lights are optional, as for a frame); n == 0 returns PTRT_OK and launches nothing. */
int ptrt_query_radiance(ptrt_ctx *ctx, const float *origins, const float *directions, uint32_t *rng_states, int n,
                        int samples, int max_depth, ptrt_radiance *out);

/* Light probes on DEVICE memory (ABI 6, addition only; no counterpart in the reference): probe p sends n_dirs rays from
 * positions[p] (n_probes*3 floats), ray (p, k) along directions[k] (n_dirs*3 floats, ONE set shared by all probes, used as
 * given and NOT normalised, for the ray and for the basis) with generator state p*n_dirs + k of `rng_states`
 * (n_probes*n_dirs*6 uint32, canonical order, advanced IN PLACE as by ptrt_query_radiance).  L(p,k), the first-hit depth and
 * the object id of ray (p, k) are exactly what ptrt_query_radiance puts into ptrt_radiance for that ray and state with the same
 * `samples` and `max_depth` -- the quirk that a primary ray takes no light sample at its first hit included -- and probe p's
 * record holds MEANS over k of these terms, all in float32:
 *     sh[i][c]          Y_i(d_k) * L_c          with d_k = (x, y, z) and, in this operation order,
 *                           Y0 = 0.282095f
 *                           Y1 = 0.488603f*y
 *                           Y2 = 0.488603f*z
 *                           Y3 = 0.488603f*x
 *                           Y4 = 1.092548f*(x*y)
 *                           Y5 = 1.092548f*(y*z)
 *                           Y6 = 0.315392f*(3.0f*(z*z) - 1.0f)
 *                           Y7 = 1.092548f*(x*z)
 *                           Y8 = 0.546274f*(x*x - y*y)
 *     mean_distance     dist = min(depth, max_distance)   (a miss has depth 1e30f)
 *     mean_distance_sq  dist*dist
 *     hit_fraction      object_id >= 0 ? 1.0f : 0.0f
 * and reserved is 0.0f.  The sum order of every quantity is part of the contract: a chunk of 64 consecutive k, padded with
 * +0.0f terms for absent k, is summed by folding halves -- v[j] + v[j + 32], then 16, 8, 4, 2, 1 --, the chunk sums are added
 * in chunk order to a total that starts at +0.0f, and the total is divided by (float)n_dirs (IEEE division, exactly rounded).
 * tests/probe_restatement.py states it in numpy.  The outputs are means: for directions uniform on the sphere the caller
 * multiplies by 4 pi to get the projection's integral (ptrt_amd.probes.sh9_irradiance does).
 * Ordering and side effects are those of ptrt_query_radiance: enqueued on the context's stream with no allocation, copy or
 * synchronisation; it touches none of the context's generator states, frame buffers, ptrt_get_stats counters or timing
 * histories; ptrt_get_option "query_pmode" reports the traversal.  One wave owns a probe, so a call with few probes and very
 * many directions fills the device better through ptrt_query_radiance.  PTRT_E_INVALID (nothing enqueued, `d_out` and the
 * states untouched) for n_probes < 0, n_dirs < 1, a NULL pointer, memory that is not the context's device memory or an
 * allocation too small (byte counts are formed in size_t), samples / max_depth outside 1..32767, or a max_distance that is
 * not positive and finite; PTRT_E_NOT_READY before geometry and materials are uploaded; n_probes == 0 returns PTRT_OK and
 * launches nothing. */
int ptrt_query_probes(ptrt_ctx *ctx, const float *d_positions, int n_probes, const float *d_directions, int n_dirs,
                      uint32_t *d_rng_states, int samples, int max_depth, float max_distance, ptrt_probe *d_out);

/* Lightmap texels on DEVICE memory: the cosine-gather irradiance query (ABI 6, addition only; no counterpart in the
 * reference).  Texel t has a position positions[t] and a normal N = normals[t] (n_texels*3 floats each; N is used as given and
 * NOT normalised -- callers pass unit normals) and gathers n_dirs rays.  Ray (t, k), every operation in float32 and separately
 * rounded:
 *     samples     u1 = samples2[2k], u2 = samples2[2k+1] (`d_samples2`: ONE set of n_dirs points in [0,1)^2 shared by all texels,
 *                 used as given); with `d_phases` (n_texels floats, the per-texel rotation; may be NULL) u2 becomes
 *                 u2 + phases[t], minus 1.0f if that sum is >= 1.0f
 *     local       r = sqrt(u1), phi = 6.28318530717958647692f * u2, (r*cos(phi), r*sin(phi), sqrt(max(0, 1 - u1))): the path
 *                 tracer's own cosine-hemisphere sample (sampling.cuh) with u1, u2 in place of generator draws, its sine and
 *                 cosine the library's deterministic ones
 *     direction   local.x*T + local.y*B + local.z*N with T, B the reference's createOrthoNormalBasis(N) (hemisphere_to_world),
 *                 its branch for a degenerate normal included
 *     origin      positions[t] + offset*N, per component: the product, then the sum
 *     state       t*n_dirs + k of `d_rng_states` (n_texels*n_dirs*6 uint32, canonical order, advanced IN PLACE as by
 *                 ptrt_query_radiance)
 * L(t,k), the first-hit depth and the object id of ray (t, k) are BY DEFINITION what ptrt_query_radiance puts into ptrt_radiance
 * for that ray and state with the same `samples` and `max_depth` -- the quirk that a caller's ray takes no light sample at its
 * first hit included.  So the direct term of the analytic lights (ptrt_upload_lights) at the texel itself and at a gather ray's
 * first hit is absent, as it is in a frame's first vertex (ptrt_query_direct, below, bakes the term at the texel, ptrt_query_bounce the term at the gather rays' first hits); emissive meshes, the sky and the environment map are seen, and the
 * lights do light every later vertex of a path.  Texel t's record holds MEANS over k:
 *     radiance[c]       L_c(t, k)                          (pi times it is the irradiance, for cosine-distributed directions)
 *     mean_distance     dist = min(depth, max_distance)    (a miss has depth 1e30f)
 *     mean_distance_sq  dist*dist
 *     hit_fraction      object_id >= 0 ? 1.0f : 0.0f
 * and reserved is 0.0f.  The sum order of every quantity is part of the contract.  Let w be the smallest power of two >= n_dirs
 * if n_dirs <= 64, else 64.  A chunk of w consecutive k, padded with +0.0f terms for absent k (selected, not computed), is
 * summed by folding halves -- v[j] + v[j + w/2], then w/4, .. 1 --, the chunk sums are added in chunk order to a total that
 * starts at +0.0f (one chunk when n_dirs <= 64), and the total is divided by (float)n_dirs (IEEE division).  For w = 64 this is
 * ptrt_query_probes's order; tests/irradiance_restatement.py states it in numpy.
 * ptrt_irradiance_rays writes exactly these origins and directions (n_texels*n_dirs*3 floats each, ray t*n_dirs + k) with one
 * small kernel on the context's stream: to the bake what ptrt_camera_rays is to a frame -- fed to ptrt_query_radiance with the
 * same states they give the per-ray records the texel's means are formed from, bit for bit.  It needs no uploaded scene, and
 * takes at most (2^31 - 1) * 256 rays per call (one thread per ray in blocks of 256; more is PTRT_E_INVALID).
 * Ordering and side effects are those of ptrt_query_probes: enqueued on the context's stream with no allocation, copy or
 * synchronisation; neither call touches the context's generator states, frame buffers, ptrt_get_stats counters or timing
 * histories; ptrt_get_option "query_pmode" reports the query's traversal, option "persist" sizes its grid.  Up to 64 directions
 * a wave owns 64/w consecutive texels; beyond, one texel, whose chunks of 64 directions it walks in order.  PTRT_E_INVALID
 * (nothing enqueued; `d_out`, the states and the ray targets untouched) for n_texels < 0, n_dirs < 1, a NULL pointer other than
 * d_phases, memory that is not the context's device memory or an allocation too small (byte counts are formed in size_t), an
 * offset that is not finite, and for the query samples / max_depth outside 1..32767 or a max_distance that is not positive
 * and finite; ptrt_query_irradiance returns PTRT_E_NOT_READY before geometry and materials are uploaded; n_texels == 0 returns
 * PTRT_OK and launches nothing. */
int ptrt_irradiance_rays(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n_texels,
                         const float *d_samples2, int n_dirs, const float *d_phases /* may be NULL */, float offset,
                         float *d_origins, float *d_directions);
int ptrt_query_irradiance(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n_texels,
                          const float *d_samples2, int n_dirs, const float *d_phases /* may be NULL */, float offset,
                          uint32_t *d_rng_states, int samples, int max_depth, float max_distance, ptrt_irradiance *d_out);

/* Lightmap texels on DEVICE memory: the direct term of the analytic lights (ptrt_upload_lights) at the texel itself -- what the
 * cosine gather above cannot see (ABI 6, addition only; no counterpart in the reference).  Texel t has P = positions[t] and
 * N = normals[t] (n_texels*3 floats each; N is used as given and NOT normalised).  The lights are light_first ..
 * light_first + light_count - 1 of the uploaded set (a caller bakes per-light layers with ranges), Q = light_count * n_shadow,
 * and term q = j*n_shadow + s is shadow sample s of light light_first + j.  Every operation in float32 and separately rounded,
 * in this order:
 *     u1, u2      samples2[2s], samples2[2s+1] (`d_samples2`: ONE set of n_shadow points in [0,1)^2 for all texels and lights,
 *                 used as given); with `d_phases` (n_texels floats; may be NULL) u2 becomes u2 + phases[t], minus 1.0f if that
 *                 sum is >= 1.0f.  Only a local light with radius > 0 reads them.
 *     L, pdf, radiance, att, light_dist
 *                 the path tracer's own light sample (sample_direct_lighting_with_mat, path_logic.cuh:311-381) with
 *                 hit.point = P, hit.normal = N, ONE light in the pick (pdf_pick = 1.0f: a sphere light's density is
 *                 1 / solid_angle above the reference's 1e-6f threshold and 1.0f below it) and u1, u2 in place of the two
 *                 draws of sample_cone_direction; attenuation, spot factor, the radius*radius / dist^2 clamp and
 *                 light_dist = 1e30f for a directional light are the reference's
 *     cos         dot(N, L)
 *     weight[c]   ((radiance[c] * att) * cos) / pdf  if cos > 0.0f && pdf > 0.0f, else +0.0f.  No soft clamp: the reference's
 *                 clamp of 500 belongs to the BSDF product, which has no part here
 *     walked      weight.x > 0 || weight.y > 0 || weight.z > 0 (a NaN weight is not walked: the reference's idiom for a
 *                 sample that adds nothing either way)
 *     origin      P + offset*N, per component: the product, then the sum (offset = 1e-4f: the bits of the path tracer's own
 *                 shadow origin)
 *     tmax        light_dist - 1e-3f
 *     blocked     walked && bvh_any_hit_tlas(origin, L, tmax): BY DEFINITION what ptrt_query_rays(PTRT_QUERY_OCCLUDED) answers
 *                 for that ray; meshes with transmission > 0.5 do not block
 *     term[c]     weight[c] if walked && !blocked, else +0.0f
 * Texel t's record holds
 *     irradiance[c]      sum over q of term[c], divided by (float)n_shadow: the sum over the lights of each light's mean
 *     lit_fraction       sum over q of (walked && !blocked ? 1.0f : 0.0f), divided by (float)Q
 *     shadowed_fraction  sum over q of (blocked ? 1.0f : 0.0f), divided by (float)Q
 * and reserved is 0.0f.  Both fractions above zero: a penumbra, or a texel some lights reach; both zero: every sample faces
 * away, lies outside a cone or has zero weight.  A light with a radius contributes radiance * solid angle (its density is
 * 1 / solid_angle): the reference's model, not renormalised.  The sum order is ptrt_query_irradiance's with Q in place of
 * n_dirs: w is the smallest power of two >= Q if Q <= 64, else 64; a chunk of w consecutive q, padded with +0.0f (selected,
 * not computed), is folded by halves -- v[j] + v[j + w/2], then w/4, .. 1 --, chunk sums are added in chunk order to a total
 * that starts at +0.0f, and one IEEE division ends each quantity.  tests/direct_restatement.py states it in numpy.
 * light_count == 0 gives rows of all-zero bytes and PTRT_OK.
 * ptrt_direct_rays writes, for ray t*Q + q, origin and L (3 floats each), tmax (1 float) and weight (3 floats) as above --
 * for rays that are not walked too, as computed, NaN included -- with one small kernel on the context's stream (one thread
 * per ray in blocks of 256, at most (2^31 - 1) * 256 rays per call).  It needs uploaded lights but no geometry.
 * Ordering and side effects are those of ptrt_query_rays: enqueued on the context's stream with no allocation, copy or
 * synchronisation, behind earlier frames, uploads (light uploads included), refits and instance updates; later frames are
 * ordered behind it; neither call touches the context's generator states, frame buffers, ptrt_get_stats counters or timing
 * histories; ptrt_get_option "query_pmode" reports the query's traversal, option "persist" sizes its grid as for the shading
 * queries; band and interleaved contexts answer for the whole scene.  PTRT_E_INVALID (nothing enqueued, every output
 * untouched) for n_texels < 0, n_shadow < 1, light_first < 0, light_count < 0, light_first + light_count beyond the uploaded
 * lights, a NULL pointer other than d_phases, memory that is not the context's device memory or an allocation too small (byte
 * counts are formed in size_t), a Q beyond 2^31 - 1 or a ray count beyond the limits above, or an offset that is not finite;
 * ptrt_query_direct returns PTRT_E_NOT_READY before geometry is uploaded; n_texels == 0 returns PTRT_OK and launches
 * nothing. */
int ptrt_direct_rays(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n_texels,
                     const float *d_samples2, int n_shadow, const float *d_phases /* may be NULL */, float offset,
                     int light_first, int light_count,
                     float *d_origins, float *d_directions, float *d_tmax, float *d_weights);
int ptrt_query_direct(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n_texels,
                      const float *d_samples2, int n_shadow, const float *d_phases /* may be NULL */, float offset,
                      int light_first, int light_count, ptrt_direct *d_out);

/* Lightmap texels on DEVICE memory: the analytic lights' ONE-BOUNCE term -- light that reaches the texel after exactly one
 * reflection off the surface a gather ray hits first.  ptrt_query_irradiance cannot see it (a caller's ray takes no light
 * sample at its first hit) and ptrt_query_direct lights the texel itself; in a room lit by a point light it is the whole
 * indirect term at max_depth 1 (ABI 6, addition only; no counterpart in the reference).  The inputs per texel are those of
 * ptrt_query_irradiance -- positions, normals, `d_samples2` with n_dirs points, `d_phases` or NULL, `offset` -- and
 * `d_shadow2` (ONE set of n_shadow points in [0,1)^2, used as given), `light_first`, `light_count`; Q = light_count * n_shadow.
 * Every operation in float32 and separately rounded, in this order:
 *     ray (t, k)  the origin and direction ptrt_irradiance_rays writes for (t, k); rd its direction
 *     hit         BY DEFINITION what ptrt_query_rays(PTRT_QUERY_CLOSEST) answers for that ray: point, normal, front_face,
 *                 mesh_index, t.  A miss adds nothing and walks nothing.
 *     throughput  (1, 1, 1); on a back-face hit multiplied by the path's Beer-Lambert factor (path_logic.cuh:823-831 with the
 *                 hit mesh's albedo and hit.t): the first half of a path vertex, its emission discarded
 *   and for term q = j*n_shadow + s, shadow sample s of light light_first + j:
 *     u1, u2      shadow2[2s], shadow2[2s+1]; with `d_phases`, u2 becomes u2 + phases[t], minus 1.0f if that sum is >= 1.0f
 *                 (the rotation ptrt_query_direct gives its samples)
 *     L, pdf, radiance, att, light_dist
 *                 the path tracer's own light sample (sample_direct_lighting_with_mat, path_logic.cuh:311-381) seen from the
 *                 hit, with ONE light in the pick (pdf_pick = 1.0f, as in ptrt_query_direct) and u1, u2 in place of the two
 *                 draws of sample_cone_direction
 *     origin      the PATH's shadow origin: hit.point + hit.normal*1e-4f if dot(hit.normal, L) > 0.0f, else
 *                 hit.point - hit.normal*1e-4f
 *     tmax        light_dist - 1e-3f
 *     bsdf        evaluateBSDF(hit, material of hit.mesh_index, L, V = -rd), the material model a frame would use
 *     direct      ((bsdf * radiance) * att) / pdf per channel -- the reference's operand order --, then
 *                 clamp_vector_soft(direct, 500).  The soft clamp is KEPT: it belongs to the BSDF product.  The reference's
 *                 mis_weight is NOT applied: an analytic light has no geometry, so no BSDF-sampled ray can reach it and there
 *                 is no second estimator to balance against; ptrt_query_direct applies none either.
 *     value       throughput * direct
 *     walked      pdf > 0.0f && (direct.x > 0 || direct.y > 0 || direct.z > 0); a NaN is not walked
 *     blocked     walked && what ptrt_query_rays(PTRT_QUERY_OCCLUDED) answers for (origin, L, tmax)
 * Ray (t, k) keeps B(t, k)[c] -- the sum over q, in q order from +0.0f, of value[c] of the terms walked and not blocked,
 * divided by (float)n_shadow --, its count of such (lit) terms and its count of blocked terms, each count converted to float.
 * Texel t's record holds
 *     radiance[c]        sum over k of B(t, k)[c] (+0.0f for a miss), divided by (float)n_dirs
 *     lit_fraction       sum over k of the lit counts, divided by (float)(n_dirs * Q)
 *     shadowed_fraction  sum over k of the blocked counts, divided by (float)(n_dirs * Q)
 *     hit_fraction       sum over k of (hit ? 1.0f : 0.0f), divided by (float)n_dirs
 * and reserved is 0.0f.  The reduction over k is EXACTLY ptrt_query_irradiance's: w, the fold by halves of a chunk padded with
 * +0.0f, chunk sums in chunk order onto +0.0f, one IEEE division.  tests/bounce_restatement.py states it in numpy.
 * light_count == 0 gives rows of all-zero bytes and PTRT_OK.
 * ptrt_bounce_terms writes the terms out for hits the caller holds: `d_hits` and `d_directions` are the n_texels*n_dirs ptrt_hit
 * records and ray directions (ray t*n_dirs + k) that ptrt_irradiance_rays and ptrt_query_rays(PTRT_QUERY_CLOSEST) make; row
 * (t*n_dirs + k)*Q + q receives origin and L (3 floats each), tmax (1 float) and value (3 floats) as above -- as computed,
 * walked or not, NaN included; a miss, or a record whose mesh_index has no uploaded material, gives a row of zeros.  One small
 * kernel on the context's stream (one thread per term in blocks of 256, at most (2^31 - 1) * 256 rows per call).  It needs
 * uploaded materials and lights, and no geometry.
 * Ordering and side effects are those of ptrt_query_direct and ptrt_query_irradiance: enqueued on the context's stream with no
 * allocation, copy or synchronisation; later frames are ordered behind it; neither call touches the context's generator
 * states, frame buffers, ptrt_get_stats counters or timing histories; ptrt_get_option "query_pmode" reports the query's
 * traversal, option "persist" sizes its grid.  PTRT_E_INVALID (nothing enqueued, every output untouched) for n_texels < 0,
 * n_dirs < 1, n_shadow < 1, light_first < 0, light_count < 0, light_first + light_count beyond the uploaded lights, a NULL
 * pointer other than d_phases, memory that is not the context's device memory or an allocation too small (byte counts are
 * formed in size_t), Q or n_dirs * Q beyond 2^31 - 1, a row count beyond the limit above, or an offset that is not finite;
 * PTRT_E_NOT_READY before geometry and materials are uploaded (ptrt_bounce_terms: materials); n_texels == 0 returns PTRT_OK
 * and launches nothing.
 * Not built: a lit first vertex inside ptrt_query_radiance or ptrt_query_probes; compaction of the lanes whose gather ray
 * missed; RT-context and tile-farm variants; a back-face fraction. */
int ptrt_bounce_terms(ptrt_ctx *ctx, const ptrt_hit *d_hits, const float *d_directions, int n_texels, int n_dirs,
                      const float *d_shadow2, int n_shadow, const float *d_phases /* may be NULL */,
                      int light_first, int light_count,
                      float *d_origins, float *d_L, float *d_tmax, float *d_values);
int ptrt_query_bounce(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n_texels,
                      const float *d_samples2, int n_dirs, const float *d_phases /* may be NULL */, float offset,
                      const float *d_shadow2, int n_shadow, int light_first, int light_count, ptrt_bounce *d_out);

/* The front of a lightmap bake: the UV charts of uploaded mesh `mesh_index` rasterised into an atlas of atlas_w x atlas_h
 * records in DEVICE memory -- the texels whose positions and normals ptrt_query_irradiance and ptrt_query_direct take.  d_uv
 * holds face_count * 6 floats on the device: the (x, y) of corners v0, v1, v2 of face f, in the face's own corner order, in
 * TEXEL units.  Texel (i, j) is record j * atlas_w + i and its centre is ((float)i + 0.5f, (float)j + 0.5f).
 * Coverage and barycentrics are one definition in fp32, every operation rounded on its own, `/` the IEEE quotient:
 *     d1 = (x1-x0, y1-y0)   d2 = (x2-x0, y2-y0)   q = (px-x0, py-y0)        A = d1x*d2y - d1y*d2x
 *     b1 = (qx*d2y - qy*d2x) / A      b2 = (d1x*qy - d1y*qx) / A      b0 = (1 - b1) - b2
 *     covered  <=>  b0 >= 0 && b1 >= 0 && b2 >= 0
 * so both windings work (the quotients carry A's sign), edges are inclusive and a NaN fails.  A face with a non-finite corner,
 * A == 0 or A NaN covers nothing; corners far outside the atlas (+-1e30) are legal.  The centres tested for a face are those of
 * columns max(floor(min x) - 1, 0) .. min(ceil(max x), atlas_w - 1) and the rows alike -- every centre inside the triangle's
 * bounds, with a texel to spare.  A covered texel's record: position = the local point (v0 + b1*e1) + b2*e2 per component from
 * the face's uploaded triangle (e1 = v1 - v0, e2 = v2 - v0 as the upload subtracted them, or as the last refit / rebuild
 * repacked them), through the mesh's world matrix if it has a transform; normal = the triangle's stored geometric normal,
 * normalize(cross(e1, e2)), with a transform normalize(normal matrix * it) -- what a front-face hit of ptrt_query_rays reports;
 * face = f; mesh = mesh_index.  tests/atlas_restatement.py states all of it in numpy.
 * Ownership is a contract: within one call the LOWEST face index covering a centre owns the texel, whatever the leaf order
 * (ptrt_build_bvh), the grid (option "persist") or the lanes per triangle (option "atlas_lanes").  clear != 0: every record
 * starts empty (mesh -1, position and normal 0).  clear == 0: d_texels holds records of earlier calls; a texel with
 * mesh >= 0 is kept whole -- earlier calls win, which is how several meshes share an atlas -- and the others are filled as
 * above.  A face that is in no leaf slot of its BVH is not rasterised (no ray can hit it either); a face in several slots
 * gives the same record.
 * Three launches on the context's stream -- prime the records, an atomic minimum of the face index per covered texel, the
 * winners' records behind the kernel boundary -- on a persistent grid over the mesh's leaf slots (option "persist" sizes it),
 * `atlas_lanes` lanes to a triangle's texel range; no allocation, copy or synchronisation; ordered like ptrt_query_rays,
 * behind uploads, refits, rebuilds and instance updates, and it leaves generator states, frame buffers, counters and timing
 * histories alone.  PTRT_E_INVALID (nothing enqueued, d_texels untouched) for a mesh_index outside the uploaded meshes,
 * atlas_w or atlas_h < 1 or a product above 2^28, a NULL pointer, d_texels not 16-byte or d_uv not 4-byte aligned, memory that
 * is not the context's device memory or an allocation too small; PTRT_E_NOT_READY before geometry is uploaded.
 * (ABI 6, addition only.) */
int ptrt_atlas_texels(ptrt_ctx *ctx, int mesh_index, const float *d_uv, int atlas_w, int atlas_h, int clear,
                      ptrt_atlas_texel *d_texels);

/* The tail of a bake: `passes` dilation passes over an atlas of float4 {r, g, b, valid} texels in DEVICE memory, d_a -> d_b ->
 * d_a ..; the result is in d_b for an odd `passes`, in d_a for an even one (the other buffer holds the pass before).  A texel
 * is valid when valid != 0.  One pass: a valid texel is copied; an invalid texel with n > 0 valid 8-neighbours inside the
 * atlas becomes the sum of their rgb -- from 0.0f, in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1), fp32,
 * each sum rounded -- divided by (float)n, with valid = 1.0f; an invalid texel with no valid neighbour is copied as it is.  A
 * pass reads only its source, so a texel filled in pass k counts as valid from pass k + 1 on.  One launch per pass on the
 * context's stream, 16-byte loads and stores, no allocation, copy or synchronisation; side effects as ptrt_atlas_texels.
 * PTRT_E_INVALID (nothing enqueued) for passes outside 1 .. 64, atlas sizes as above, a NULL or not 16-byte aligned pointer,
 * buffers that overlap, memory that is not the context's device memory or too small.  Needs no scene.  (ABI 6, addition only.) */
int ptrt_atlas_dilate(ptrt_ctx *ctx, float *d_a, float *d_b, int atlas_w, int atlas_h, int passes);

/* Between scatter and dilation: `passes` (1 .. 8) passes of an edge-aware a-trous filter over a baked atlas of float4
 * {r, g, b, valid} texels in DEVICE memory, guided by the atlas's own records d_texels (ptrt_atlas_texels' output, atlas_w *
 * atlas_h of them, only read): light is averaged over texels that are close in the world, near the centre's tangent plane and
 * face the same way, so it does not bleed round a crease or between charts that are neighbours in the atlas only.  The image
 * goes d_a -> d_b -> d_a ..; the result is in d_b for an odd `passes`, in d_a for an even one (the other buffer holds the pass
 * before) -- ptrt_atlas_dilate's rule.  Pass s (from 0) has step = 1 << s.
 * One pass is ONE definition in fp32, every operation rounded on its own (no contraction), `/` the IEEE quotient.  For texel
 * p = (i, j), G = d_texels[p], C = src[p]:
 *   G.mesh < 0 or C.valid == 0 (a texel is valid when valid != 0, as for ptrt_atlas_dilate):  dst[p] = C, its 16 bytes copied.
 *   Otherwise num = (0, 0, 0), den = 0, and the 25 taps dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), in that order, at
 *   q = (i + dx*step, j + dy*step).  A tap outside the atlas, one with Gq.mesh < 0 and one with Cq.valid == 0 is skipped -- by
 *   selection, never by a product with zero: a NaN or an infinity in a skipped tap's colour or guide reaches nothing.  Else
 *       h  = K[|dx|] * K[|dy|]                     K = {0.375, 0.25, 0.0625}: the B3 spline, every product exact
 *       e  = Gq.position - G.position              per component
 *       d2 = (e.x*e.x + e.y*e.y) + e.z*e.z         x = 1 - d2 / rr          wd = x > 0 ? x : 0
 *       pd = (G.n.x*e.x + G.n.y*e.y) + G.n.z*e.z   y = 1 - (pd*pd) / pp     wp = y > 0 ? y : 0
 *       c  = (G.n.x*Gq.n.x + G.n.y*Gq.n.y) + G.n.z*Gq.n.z      c = c > 0 ? c : 0      then normal_power times  c = c*c
 *       w  = ((h * wd) * wp) * c
 *   with rr = r*r, r = sigma_distance * (float)step, and pp = sigma_plane * sigma_plane (not scaled by the step), formed in
 *   fp32 on the host.  normal_power 0 is the plain cosine, 7 its 128th power.  If !(w > 0) the tap is skipped -- a NaN weight
 *   ends here --; otherwise num += w * Cq.rgb per channel (the product rounded, then the sum) and den += w.
 *   den == 0 (a centre with a zero normal):  dst[p] = C copied.  Otherwise dst[p] = {num.r / den, num.g / den, num.b / den,
 *   C.valid}.
 * Normals are expected to be unit vectors, as ptrt_atlas_texels writes them: a longer one can take c*c*.. to infinity, and
 * infinity / infinity is a NaN by the arithmetic above.
 * tests/atlas_filter_restatement.py states all of it in numpy.  One launch per pass on the context's stream; no allocation,
 * copy or synchronisation; needs no scene; ordering and side effects are ptrt_atlas_dilate's: generator states, frame buffers,
 * counters and both timing histories are left alone.  Option "atlas_filter_tile" chooses between two shapes of a pass with the
 * same bytes.  PTRT_E_INVALID (nothing enqueued, both buffers untouched) for passes outside 1 .. 8, normal_power outside
 * 0 .. 7, a sigma that is not finite or <= 0, an rr (of any of the passes) or pp that is not finite or is zero in fp32, atlas
 * sizes outside ptrt_atlas_dilate's, a NULL or not 16-byte aligned pointer, d_a and d_b overlapping each other or d_texels,
 * memory that is not the context's device memory or too small (byte counts in size_t).  (ABI 6, addition only.) */
int ptrt_atlas_filter(ptrt_ctx *ctx, const ptrt_atlas_texel *d_texels, float *d_a, float *d_b, int atlas_w, int atlas_h, int passes,
                      float sigma_distance, float sigma_plane, int normal_power);

/* The consumer of a bake: the atlas ptrt_atlas_dilate leaves, read back at ray hits.  Everything is in DEVICE memory:
 *   d_charts       n_chart_faces * 6 floats, the layout of ptrt_atlas_texels' d_uv -- the (x, y) of corners v0, v1, v2 of a face in
 *                  texel units -- with the charts of several meshes concatenated;
 *   d_chart_first  one int32 per uploaded mesh: the index in d_charts of that mesh's face 0; negative: the mesh has no lightmap;
 *   d_image        atlas_w * atlas_h float4 {r, g, b, valid};
 *   mode           PTRT_LIGHTMAP_NEAREST or PTRT_LIGHTMAP_BILINEAR.
 * ptrt_atlas_sample answers for n ptrt_hit records H of the kind ptrt_query_rays(PTRT_QUERY_CLOSEST) writes; ptrt_query_lightmap
 * traces n rays itself, as that query would, and answers for their hits without the 64-byte records ever being written: the
 * same bytes with one launch less and 128 bytes less traffic per ray.  One ptrt_lightmap_sample per record or ray.
 * The sample is ONE definition in fp32, every operation rounded on its own (no contraction), `/` the IEEE quotient:
 *   1. H.hit == 0 (a miss):  {0, 0, 0,  0,  0, 0,  -1, -1}.
 *   2. m = H.mesh_index, f = H.face_index, first = d_chart_first[m].  If first < 0, f < 0 or first + f >= n_chart_faces (the sum
 *      in 64 bits) there is no chart:  {0, 0, 0,  0,  0, 0,  f, m}.  The range check is part of the definition -- the table is
 *      device memory the host cannot vet without a synchronisation, and a bad table must not read outside d_charts.  So is, for
 *      the same reason, a record of ptrt_atlas_sample whose m is not an uploaded mesh (m < 0 or m >= the mesh count): no chart,
 *      and d_chart_first is not read.
 *   3. (x0, y0, x1, y1, x2, y2) = d_charts[(first + f) * 6 ..];  b0 = (1 - H.u) - H.v;  x = (b0*x0 + H.u*x1) + H.v*x2, y likewise.
 *      H.u belongs to corner v1 and H.v to v2 -- the triangle test's u multiplies e1 -- : the barycentrics ptrt_atlas_texels puts
 *      through (v0 + b1*e1) + b2*e2, so the texel whose centre a chart maps to a surface point is the one a hit at that point
 *      finds.  If x or y is not finite:  {0, 0, 0,  0,  x, y,  f, m}.
 *   4. A tap (i, j) is usable iff 0 <= i < atlas_w, 0 <= j < atlas_h (integers) and d_image[j * atlas_w + i].valid != 0.  Taps are
 *      skipped by selection, never by a product with zero: a NaN or an infinity in an unusable texel reaches nothing
 *      (ptrt_atlas_filter's rule).  Taps are NOT clamped at the atlas border; they are skipped and the rest renormalised.
 *        NEAREST   fi = floor(x), fj = floor(y).  The tap (fi, fj), if usable: rgb = the texel's three words copied, weight = 1;
 *                  otherwise rgb = 0 and weight = 0.
 *        BILINEAR  tx = x - 0.5f, ty = y - 0.5f;  fi = floor(tx), fj = floor(ty);  fx = tx - fi, fy = ty - fj;  gx = 1 - fx,
 *                  gy = 1 - fy.  The taps, in this order: (i0, j0) with w = gx*gy, (i0+1, j0) with fx*gy, (i0, j0+1) with gx*fy,
 *                  (i0+1, j0+1) with fx*fy.  A usable tap with w > 0 adds num += w * rgb per channel (the product rounded, then
 *                  the sum) and den += w.  den > 0: rgb = num / den, weight = den; otherwise both are 0.
 *      Before any conversion to an integer, fi or fj outside [-1, 2^28] -- compared as floats, as the rasteriser does -- means no
 *      tap is usable: an atlas has at most 2^28 texels, so such a value has none anyway.
 *   5. The record is {rgb, weight, x, y, f, m}.
 * A hit on a face's back side samples the same texel as one on its front: the bake's normal is the front side's, and a caller
 * who cares reads front_face from ptrt_query_rays.  tests/lightmap_sample_restatement.py states all of it in numpy.
 * Ordering and side effects are ptrt_query_rays': enqueued on the context's stream; no allocation, copy or synchronisation;
 * generator states, frame buffers, counters and both timing histories are left alone; ptrt_query_lightmap walks the traversal a
 * frame would (ptrt_get_option "query_pmode" says which).  PTRT_E_INVALID (nothing enqueued, d_out untouched) for n < 0,
 * n_chart_faces < 1, atlas sizes outside ptrt_atlas_dilate's, a mode other than the two, a NULL pointer, d_image, d_out or d_hits
 * not 16-byte aligned, d_charts, d_chart_first, d_origins or d_directions not 4-byte aligned, memory that is not the context's
 * device memory or too small (d_chart_first: one entry per uploaded mesh; byte counts in size_t), d_out overlapping an input.
 * PTRT_E_NOT_READY before geometry is uploaded (ptrt_atlas_sample needs the scene for the mesh count only); n == 0 is PTRT_OK.
 * (ABI 6, additions only.) */
#define PTRT_LIGHTMAP_NEAREST 0
#define PTRT_LIGHTMAP_BILINEAR 1
int ptrt_atlas_sample(ptrt_ctx *ctx, const ptrt_hit *d_hits, int n, const float *d_charts, int n_chart_faces,
                      const int32_t *d_chart_first, const float *d_image, int atlas_w, int atlas_h, int mode,
                      ptrt_lightmap_sample *d_out);
int ptrt_query_lightmap(ptrt_ctx *ctx, const float *d_origins, const float *d_directions, int n, const float *d_charts,
                        int n_chart_faces, const int32_t *d_chart_first, const float *d_image, int atlas_w, int atlas_h,
                        int mode, ptrt_lightmap_sample *d_out);

/* The consumer of a probe bake: a regular grid of ptrt_probe records -- what ptrt_query_probes leaves for positions laid out as
 * `volume` says -- read at surface points.  d_probes (nx*ny*nz records) and the arrays are DEVICE memory; `volume` is host memory.
 * ptrt_probe_sample answers for n points P = d_positions[i] with normals N = d_normals[i] (n*3 floats each); ptrt_query_probe_light
 * traces n rays itself, as ptrt_query_rays(PTRT_QUERY_CLOSEST) would, and answers for the `point` and `normal` (the face-forwarded
 * one) that query would have written -- formed by the same device function -- with the hit's face f and mesh m filled in: the bytes
 * of ptrt_probe_sample over those two columns, in one launch and without the 64-byte records.  One ptrt_probe_light per point.
 * The record is ONE definition in fp32, every operation rounded on its own (no contraction), `/` and sqrt the IEEE ones, sums in
 * the written order:
 *   1. A miss (ptrt_query_probe_light only):  {0, 0, 0,  0,  -1, 0,  -1, -1}.
 *   2. P has a non-finite component: no cell,  {0, 0, 0,  0,  -1, 0,  f, m}.  Memory safety depends on P alone; N is used as given,
 *      NOT normalised, and a non-finite N may give non-finite colours but never a read outside d_probes.
 *   3. The cell.  Per axis a:  g = (P[a] - origin[a]) / spacing[a];  g = min(max(g, 0), (float)(counts[a] - 1));  i0 = (int)floor(g);
 *      i1 = min(i0 + 1, counts[a] - 1);  f = g - (float)i0.  Points outside the volume are clamped to its faces.  `cell` is the
 *      row of (i0x, i0y, i0z).
 *   4. The basis at N, once per point:  B_i = K_i * Y_i(N) with Y_i exactly as ptrt_query_probes has it above (the same six-digit
 *      constants, the same operation order) and K_0 = 39.478418f (4 pi * pi), K_1..3 = 26.318945f (4 pi * 2 pi / 3),
 *      K_4..8 = 9.869604f (4 pi * pi / 4): the factor that turns ptrt_query_probes' means into projection integrals, times the
 *      cosine lobe's per band.
 *   5. The corners c = 0..7 in that order; bit 0 of c selects i1 on x, bit 1 on y, bit 2 on z.  wt = (wx*wy)*wz, each factor f or
 *      1 - f of its axis.  A corner with wt <= 0 is skipped BY SELECTION, never by a product with zero -- whatever its record holds
 *      reaches nothing (ptrt_atlas_filter's rule) and it is not loaded.  On an axis with one probe both corners name the same row
 *      and the second has weight 0.
 *        TRILINEAR   w = wt.
 *        VISIBILITY  Q = origin + (float)idx * spacing (the product rounded, then the sum);  Pb = P + normal_bias * N;  V = Q - Pb;
 *                    r2 = (Vx*Vx + Vy*Vy) + Vz*Vz;  r = sqrt(r2);  D = r > 0 ? V / r : 0.
 *                    Facing:      c = (dot(D, N) + 1) * 0.5f, the dot summed as r2 is;  wf = c*c + 0.2f.
 *                    Visibility:  mean = rec.mean_distance;  var = fabs(rec.mean_distance_sq - mean*mean);  wv = 1 when r <= mean;
 *                                 otherwise d = r - mean, ch = var / (var + d*d), wv = (ch*ch)*ch  (Chebyshev's bound, cubed).
 *                    w = wf * wv;  if w < 0.2f then w = w * ((w*w) / 0.04f);  then w = w * wt.
 *      A corner whose w is not > 0 is skipped by selection (a NaN too).  A used corner: per channel E_c = acc after acc = +0.0f,
 *      acc = acc + B_i * sh[i][c] for i = 0..8;  num_c += w * E_c;  den += w;  bit c of `used` is set.
 *   6. den > 0: irradiance_c = num_c / den, replaced by +0.0f where it is < 0 (SH ringing), weight = den; otherwise both are 0.
 *      The record is {irradiance, weight, cell, used, f, m}.
 * tests/probe_sample_restatement.py states all of it in numpy.  ptrt_amd.probes.ProbeVolume.positions() forms Q, so probes baked
 * there sit exactly where the sampler assumes.  Not built: a per-probe validity or back-face state, probe relocation, RT-context
 * and tile-farm variants.
 * Ordering and side effects are ptrt_query_rays': enqueued on the context's stream; no allocation, copy or synchronisation;
 * generator states, frame buffers, counters and both timing histories are left alone; ptrt_query_probe_light walks the traversal a
 * frame would (ptrt_get_option "query_pmode" says which).  PTRT_E_INVALID (nothing enqueued, d_out untouched) for n < 0, a NULL
 * pointer, a count < 1 or a product of the counts above 2^24 (formed in 64 bits; (float)idx stays exact), a spacing that is not
 * positive and finite, a non-finite origin, a normal_bias that is negative or not finite, a mode other than the two, d_probes or
 * d_out not 16-byte aligned, a float array not 4-byte aligned, memory that is not the context's device memory or too small (byte
 * counts in size_t), d_out overlapping an input.  PTRT_E_NOT_READY before geometry is uploaded (ptrt_query_probe_light only);
 * n == 0 is PTRT_OK with no launch.  (ABI 6, additions only.) */
#define PTRT_PROBES_TRILINEAR 0
#define PTRT_PROBES_VISIBILITY 1
int ptrt_probe_sample(ptrt_ctx *ctx, const float *d_positions, const float *d_normals, int n, const ptrt_probe_volume *volume,
                      const ptrt_probe *d_probes, int mode, float normal_bias, ptrt_probe_light *d_out);
int ptrt_query_probe_light(ptrt_ctx *ctx, const float *d_origins, const float *d_directions, int n, const ptrt_probe_volume *volume,
                           const ptrt_probe *d_probes, int mode, float normal_bias, ptrt_probe_light *d_out);

/* The primary rays ptrt_render(frame_index, ..) gives sample `sample` of every pixel of the context's rows -- TAA and
 * blue-noise jitter of frame_index + sample, the context's camera, the render size if one is set -- written by one small
 * kernel on the context's stream into DEVICE memory: rows*W*3 floats each (render_w*render_h*3 at a reduced render size),
 * ray yl*W + x, the order of PTRT_BUF_ACCUM.  The frame's own device functions make them.  The starting point of a custom
 * camera, and what lets ptrt_query_radiance be compared with a frame.  PTRT_E_INVALID for a thin lens (lens_radius > 0:
 * that ray's lens sample belongs to the pixel's generator stream, not to the camera), a negative frame_index or sample, a
 * NULL pointer or memory that is not the context's device memory.  (ABI 6, addition only.) */
int ptrt_camera_rays(ptrt_ctx *ctx, int frame_index, int sample, float *d_origins, float *d_directions);

/* n generator states in the canonical order {d, v0..v4} for subsequences first_subsequence .. first_subsequence + n - 1 of
 * `seed`, offset 0, written into DEVICE memory (n*6 uint32) by one kernel on the context's stream: curand_init(seed,
 * subsequence, 0, ..) as ptrt_reset_rng computes it for pixel `subsequence` (init_curand_kernel, scene_kernels.cuh:26-35).
 * PTRT_E_INVALID for n < 0, NULL, memory that is not the context's device memory, or a last subsequence of 2^40 or more;
 * n == 0 returns PTRT_OK.  (ABI 6, addition only.) */
int ptrt_init_rng_states(ptrt_ctx *ctx, unsigned long long seed, unsigned long long first_subsequence, int n,
                         uint32_t *d_states);

/* The body of Scene::render_to_device_wireframe (scene.cuh:1211-1245): render_kernel_wireframe
 * (scene_kernels.cuh:53-117, wireframeMode true) over the full width x height -- the render size of the path tracer,
 * bloom and the denoiser play no part.  Per pixel: the RNG-free Camera::get_ray(s, t) (camera.cuh:173-199, device branch:
 * a thin lens takes its offset from random_in_unit_disk_hash), one closest hit; a hit with u, v or 1 - u - v below
 * `thickness` is an edge, coloured by its mesh's emission if emission.x > 0 and white otherwise; every other pixel shows
 * sampleSky (render_utils.cuh:115-137); then c / (c + 1), powf(c, 1 / 2.2), * 255.99 into RGB8, bottom-up.
 * `out_rgb8` / `out_is_device` as for ptrt_render (PTRT_OUT_HOST synchronous, PTRT_OUT_DEVICE the context's rows,
 * PTRT_OUT_DEVICE_FRAME the whole frame); a target is required.  Enqueued on the context's stream, behind any earlier
 * ptrt_render of the context (pipelined ones included).  Touches no generator state, accumulation, G-buffer or
 * PTRT_BUF_RGB8 image, no counter of ptrt_get_stats and no timing history: path frames before and after it are the
 * frames they would be without it.  PTRT_E_INVALID for an interleaved context (the tile farm has no wireframe view),
 * PTRT_E_NOT_READY before geometry and materials are uploaded.  (ABI 6, addition only.) */
int ptrt_render_wireframe(ptrt_ctx *ctx, float thickness, void *out_rgb8, int out_is_device);

/* The baked-light view: the scene lit by what was baked for it -- a lightmap atlas (ptrt_query_lightmap's four arguments), a probe
 * volume (ptrt_query_probe_light's), both or neither -- as one frame, in one launch: primary ray, closest hit, the two samplers,
 * the context's own materials, the path frame's tonemap.  `view` is HOST memory and is copied into the launch; the pointers in
 * it are DEVICE memory.  d_image NULL: no lightmap (its other fields are not looked at); d_probes NULL: no probes; with neither
 * the frame shows emission and sky only.  Like the wireframe view it is always the full width x height: the render size of the
 * path tracer, bloom and the denoiser play no part.
 * A pixel is ONE definition in fp32, every operation rounded on its own (no contraction), `/` the IEEE quotient.  For pixel
 * (x, y) of the context's rows:
 *   1. The primary ray is the one ptrt_camera_rays(frame_index, 0) writes for the pixel when no reduced render size is set: the
 *      TAA and blue-noise jitter of frame_index over the full width and height, the pinhole camera.
 *   2. The closest hit is what ptrt_query_rays(PTRT_QUERY_CLOSEST) answers for that ray.
 *   3. A miss:  c = use_sky ? sampleSky(direction) : 0  (ptrt_set_sky, ptrt_set_env_map).
 *   4. A hit on face f of mesh m at (u, v): the irradiance E is, in this order,
 *        the `rgb` of ptrt_query_lightmap's sample        where a lightmap is given and the sample's weight > 0;
 *        the `irradiance` of ptrt_query_probe_light's      otherwise, where a volume is given and its weight > 0: the sample at
 *                                                          the hit's `point` and face-forwarded `normal`;
 *        +0                                                otherwise.
 *      The probe sample runs only in pixels the lightmap left empty -- a mesh without a chart (d_chart_first[m] < 0: a moving
 *      object is lit by the volume, a baked wall by its atlas), a texel that is invalid or outside the atlas, a non-finite chart
 *      point -- and the skip is by selection: what an unused sample holds reaches nothing.  A NaN weight is not > 0.
 *   5. c = (albedo_m * E) / 3.14159265f + emission_m per channel -- the product, the quotient, then the sum -- with albedo_m and
 *      emission_m the context's materials as uploaded (ptrt_upload_materials): ptrt_amd.lightmap.shade_samples' three operations.
 *   6. The outputs, each optional, at least one of out_rgb8 and d_hdr given:
 *        d_hdr                        rows*W*3 floats, pixel yl*W + x, the order of PTRT_BUF_ACCUM:  c;
 *        d_normal, d_depth,           rows*W*3 floats, rows*W floats, rows*W int32, the layouts ptrt_post_frame takes: what a frame
 *        d_object_id                  keeps of a first hit -- the face-forwarded normal or zeros, t or 1e30f, the mesh or -1;
 *        out_rgb8                     the path frame's tonemap of c (ACES + sRGB), bottom-up, as for ptrt_render_wireframe:
 *                                     PTRT_OUT_HOST synchronous, PTRT_OUT_DEVICE the context's rows, PTRT_OUT_DEVICE_FRAME the
 *                                     whole frame (a band context writes its rows where they belong in it).
 * tests/baked_view_restatement.py states 3 to 6 in numpy over the rows of the entry points named above.
 * Ordering and side effects are the wireframe view's: enqueued on the context's stream, behind any earlier ptrt_render of the
 * context (pipelined ones included); touches no generator state, accumulation, G-buffer or PTRT_BUF_RGB8 image, no counter of
 * ptrt_get_stats and no timing history.  The grid is the device queries' -- persistent one-wave workgroups striding over the
 * frame's 8x8 tiles, the traversal a frame would walk (ptrt_get_option "query_pmode"); option "persist" sizes it.
 * PTRT_E_INVALID (nothing enqueued, every output untouched) for an interleaved context, a thin lens (as ptrt_camera_rays), a
 * negative frame_index, a NULL view, no target at all (out_rgb8 and d_hdr both NULL, or an out_is_device outside the three), a
 * lightmap half ptrt_query_lightmap would refuse, a probe half ptrt_query_probe_light would refuse, an output that is not the
 * context's device memory, is too small, is not 4-byte aligned or overlaps an input or another output (byte counts in size_t).
 * PTRT_E_NOT_READY before geometry and materials are uploaded, or with fewer materials than meshes.  Not built: more than one
 * atlas or volume per frame, a reduced render size, exposure, RT-context and tile-farm variants.  (ABI 6, addition only.) */
typedef struct ptrt_baked_view {           /* HOST memory, copied into the launch */
    const float *d_charts; int32_t n_chart_faces; const int32_t *d_chart_first;
    const float *d_image; int32_t atlas_w, atlas_h, lightmap_mode;   /* d_image NULL: no lightmap */
    ptrt_probe_volume volume; const ptrt_probe *d_probes;
    int32_t probe_mode; float normal_bias;                           /* d_probes NULL: no probes  */
    float *d_hdr, *d_normal, *d_depth; int32_t *d_object_id;         /* each may be NULL          */
} ptrt_baked_view;
int ptrt_render_baked(ptrt_ctx *ctx, int frame_index, const ptrt_baked_view *view, void *out_rgb8, int out_is_device);

/* counters accumulated by ptrt_render since the last call (reset on read);
 * only maintained when ptrt_set_option(ctx,"count_rays",1). */
int ptrt_get_stats(ptrt_ctx *ctx, ptrt_stats *out);

/* Tile farm, presenting rank: steps 3-7 of Scene::render_to_device (motion vectors,
 * Denoiser::denoise, bloom, tonemap; scene.cuh:1103-1208) of a FULL-FRAME context over a frame whose
 * HDR image and G-buffers were rendered by other contexts (bands) and gathered into DEVICE memory:
 * accum/normal width*height*3 floats, depth width*height floats, object_id width*height ints, top-down,
 * i.e. the bands' ptrt_device_buffer contents concatenated in row order.  Camera, previous view-projection
 * and the denoiser/bloom switches are the context's own.  PTRT_E_INVALID for a band context, a reduced
 * render size, or when neither stage is enabled.  Object ids are any `int32_t` but `INT_MIN`, which the
 * a-trous staging uses for "outside the image or sky" (`AT_OUTSIDE`): a pixel with that id would be dropped
 * from every tap of every pass. */
int ptrt_post_frame(ptrt_ctx *ctx, const float *accum, const float *normal, const float *depth,
                    const int32_t *object_id, void *out_rgb8, int out_is_device);

/* ---- the tile farm below the C ABI: one process, the GPUs of one node --------------------------------
 * The reference has no multi-GPU code; a C++ application built on the Scene mirror farms a frame by holding one
 * band / strip context per GPU (ptrt_create / ptrt_create_interleaved with the device of each) and handing them
 * to a farm, which gathers their RGB8 images onto the device of the FIRST context -- the presenting device, whose
 * viewer maps the frame (rtgl::map_pbo_device_ptr).  Contexts on the presenting device are copied device-to-device;
 * contexts on other devices send with ncclSend / ncclRecv over RCCL (xGMI), one grouped call per frame; strips are
 * scattered to their places.  No host synchronisation inside a frame (out_is_device != 0); a context's next render
 * waits on its own stream until its image has been taken.  The contexts stay the caller's (uploads, options, destroy
 * them AFTER the farm); they must tile the frame exactly once, else PTRT_E_INVALID.
 *   ptrt_farm_render  = ptrt_render(ctx, frame, spp, depth, NULL, 0) on every context + ptrt_farm_gather
 *   ptrt_farm_gather  = gather of the images the contexts hold (for callers that render through the Scene mirror)
 *   ptrt_farm_transport: "device-copy" (all contexts on one device), "rccl", or "peer-copy": hipMemcpyPeerAsync of a remote
 *                     context's image onto the presenting device, on the farm's stream behind the context's render -- no RCCL
 *                     involved (SURVEY 8(e) names it as the alternative).  "peer-copy" is what a farm uses when librccl cannot be
 *                     loaded or ncclCommInitAll fails, with PTRT_FARM_TRANSPORT=peer in the environment, or after
 *                     ptrt_farm_set_option(farm, "transport", 1) (0 = back to RCCL, refused if its communicators never came
 *                     up).  Errors: ptrt_last_error(NULL).
 * The "rccl" transport is UNVERIFIED ON HARDWARE (every test so far ran on a one-GPU box); "peer-copy" has run with equal source
 * and destination device only (PTRT_FARM_FORCE_REMOTE=1: a test hook that makes a farm treat every part but the first as remote).  A presentation-ring slot as the
 * device target (rtgl::map_pbo_device_ptr) is recognised: its download is ordered behind the gather's copies. */
typedef struct ptrt_farm ptrt_farm;
int ptrt_farm_create(ptrt_ctx *const *contexts, int n_contexts, ptrt_farm **out);
int ptrt_farm_bands(const ptrt_farm *farm);
const char *ptrt_farm_transport(const ptrt_farm *farm);
/* ABI 6: 1 if part `part` sits on the presenting device (it may render straight into the frame the gather assembles:
 * ptrt_render(..., frame, PTRT_OUT_DEVICE_FRAME)), 0 if its image has to travel (render it with a NULL target) */
int ptrt_farm_part_is_local(const ptrt_farm *farm, int part);
int ptrt_farm_render(ptrt_farm *farm, int frame_index, int spp, int max_depth, void *out_rgb8, int out_is_device);
int ptrt_farm_gather(ptrt_farm *farm, void *out_rgb8, int out_is_device);
/* ABI 5.  The per-part host work of a frame runs on one worker thread per context (a ptrt_render costs 20-50 us of host
 * time; eight in a row would be the same order as an eighth of a frame on the GPU):
 *   ptrt_farm_parallel   fn(i, user) for every context i at once, each on its own thread (the caller's takes part 0); returns
 *                        when all are back; fn must not throw.  ptrt_farm_render uses it for its ptrt_render calls, the
 *                        C++ TileFarm for its Scene::render_to_device calls.
 *   ptrt_farm_host_us    host time (us) of the caller's thread inside the last ptrt_farm_render
 *   ptrt_farm_device_frame  the device frame a gather into (out_rgb8, out_is_device) assembles: out_rgb8 itself, or the
 *                        farm's own frame when the target is host memory.  A context on the presenting device that rendered
 *                        straight into it (ptrt_render(..., frame, PTRT_OUT_DEVICE_FRAME), as ptrt_farm_render makes them do)
 *                        is not copied by the gather, only waited for
 *   ptrt_farm_set_option "parallel" 0|1 (default 1), "spin_us" (a worker polls that long for the next frame before it
 *                        sleeps; default 2000), "transport" 0|1 (see ptrt_farm_transport) */
int ptrt_farm_parallel(ptrt_farm *farm, void (*fn)(int part, void *user), void *user);
double ptrt_farm_host_us(const ptrt_farm *farm);
void *ptrt_farm_device_frame(ptrt_farm *farm, void *out_rgb8, int out_is_device);
int ptrt_farm_set_option(ptrt_farm *farm, const char *name, long long value);
int ptrt_farm_sync(ptrt_farm *farm);
void ptrt_farm_destroy(ptrt_farm *farm);

/* tuning / diagnostics knobs, by name; unknown names return PTRT_E_INVALID.  None changes a bit of
 * any output (tests force every value and compare with the oracle):
 *   count_rays 0|1        maintain the ptrt_get_stats counters
 *   force_geom -1..2      force a more general traversal variant       force_full 0|1  all material branches
 *   pair_trace 0|1        (ray, mesh) pair compaction                  pair_split 0|1  lanes per pair in partial batches
 *   fetch_min 0..64       idle lanes before the pair queue refills     leaf_pairs 0|1  compacted leaf phase
 *   leaf_min 1..64        lanes waiting at a leaf that end the descent steal 0..64     shadow-ray subtree stealing
 *   csteal 0..64          PMODE 2 closest hit: verified subtree stealing (2).  Once the pair queue is empty an idle lane takes the
 *                         BOTTOM entry of a busy walk's stack -- what that walk would visit last -- with a copy of its ray and limit,
 *                         walks it and merges what it finds; the node loop yields every `csteal` steps while lanes idle.  A thief's hit
 *                         closer than its own leaf box's entry, or two walks of one (ray, mesh) pair reporting the same distance, mark
 *                         the ray, which is then traced again without stealing: same bits.  csteal_min: node steps a
 *                         walk must have taken before it is stolen from (0); csteal_follow 0|1: a thief keeps taking its victim's
 *                         limit (1); csteal_leaf_min 1..64: leaf_min of a stealing phase (32).  0: off (showcase 3.60 -> 3.33 ms).
 *   lds_nodes 0|1         PMODE 2 in 256-thread workgroups sharing an LDS copy of the BLAS top levels
 *   merged -1|0|1         one traversal per loop iteration: a light sample's shadow ray rides with the next extension ray;
 *                         -1 (default): both shapes (equal bit for bit) take turns over a scene's frames 4-9, three samples
 *                         each; the merged one stays only if its median kernel time is at least 0.5 % below the separate-phase
 *                         default's.  The decision, at frame 10, is the ONE place where the otherwise asynchronous ptrt_render
 *                         blocks the host (a hipEventSynchronize on frame 9, once per scene and setting); set merged to 0 or 1
 *                         before the first frame to opt out.  Never taken while the stream is being captured into a hipGraph.
 *   stage 0..7            PMODE 1: shading inputs kept in LDS (0 none; else jitter inputs, |1 light records, |2 material records)
 *   pipeline 0|1, split 1..4   frame pipelining (default 1, 2).  A frame whose launch need not wait for the stream is dealt, by rows
 *                         of 8x8 tiles, to `split` launches on auxiliary streams of the context; launch i follows launch i of the
 *                         previous frame (the same pixels) and the frame is joined onto the context's stream by events, so
 *                         WHAT FOLLOWS ptrt_render ON THE STREAM STILL FOLLOWS THE FRAME -- but the frame itself may start while
 *                         the previous frame's last waves drain and while what the caller enqueued on the stream AFTER the
 *                         previous ptrt_render call still runs; it waits for everything that was on the stream when that
 *                         previous call was made, i.e. for the consumers of every frame but the last
 *                         (Cornell 1080p 1.81 -> 1.68 ms, showcase 3.85 -> 3.57).  Only when nothing else can have a claim on
 *                         what the frame reads or overwrites: a DEVICE target other than the previous frame's (double buffering:
 *                         whatever consumes the previous target on the stream is still entitled to it), no reduced render
 *                         size (with the denoiser or bloom the context keeps two sets of HDR image and G-buffers and
 *                         alternates, so that a frame's post chain and the next frame's trace do not share one), no ptrt_* call since the previous ptrt_render other than the host-only ones
 *                         (ptrt_set_camera / _sky / _option / _prev_view_proj, ptrt_get_option, ptrt_sync, ptrt_last_error,
 *                         ptrt_set_bloom(0)), no pointer from ptrt_device_buffer in the caller's hands, not while the loop shape is
 *                         being sampled or the stream captured.  Any other frame is ONE launch
 *                         ordered behind the stream, as with pipeline = 0.  ptrt_get_option "pipelined" says which the last one was.
 *   refill 0|1|2, persist N   PMODE 1, lane refill: the launch is a grid of persistent waves (`persist` per CU; 0 = what the
 *                         kernel's occupancy holds) that draw the launch's 8x8 tiles from a queue, and a lane whose pixel is finished
 *                         takes the next pixel instead of idling until the slowest pixel of its tile is done (18 % of the
 *                         lane-iterations of a 1080p Cornell frame); the image is tonemapped by a pass behind the launch.  Which lane
 *                         renders a pixel changes nothing in it: same bits.  1 (default): where it was measured to pay -- frames that
 *                         overlap their predecessor ("pipeline"), simple materials, no post chain, spp x bounces >= 16, at least two
 *                         tiles per persistent wave (1080p 4 spp 4 bounces 1.67 -> 1.63 ms, 8 bounces 2.12 -> 1.89, 4K 6.65 -> 6.27);
 *                         2: wherever PMODE 1 runs; 0: never.  ptrt_get_option "refilled" says what the last frame did.
 *                         ticket_tiles 1..16: consecutive tiles per draw from the queue (1; more only pays where the counter
 *                         itself binds -- 1 spp: 0.61 -> 0.49 ms with 4, still behind the one-tile-per-wave kernel's 0.43).
 *                         `persist` N > 0 also sizes the persistent grid of ptrt_query_radiance, ptrt_query_probes, ptrt_query_irradiance, ptrt_query_direct and ptrt_query_bounce: N one-wave workgroups per CU
 *                         instead of what the kernel's occupancy holds (tests: a grid smaller than the batch's chunks).
 *   sample_sync -1|0|1    the lanes of a wave start their samples together (1) instead of each as soon as its path has ended (0):
 *                         the wave's lanes then sit at the same bounce, the light-sample phases are skipped by the whole wave at a
 *                         first hit and the primary rays are made once per sample for 64 lanes; lanes wait for the sample's
 *                         longest path.  Same bits.  -1 (default): on where it was measured to pay -- at most 4 bounces (Cornell
 *                         1.76 -> 1.64 ms, 136 meshes 15.9 -> 14.8, the fluid frame -3 %, scenes of short paths even; 5 bounces and more lose).
 *                         ptrt_get_option "sample_sync_eff" says what the last frame did.
 *   pm1_dense_roots -1|0|1   PMODE 1: a trace whose live rays fill at most half the wave deals its root-box tests over all 64
 *                         lanes -- 2 or 4 meshes per slab round instead of one.  Same pair list, same bits.
 *                         -1 (default): on with at least four meshes in the leaf, decided on the host from the scene (Cornell 1080p
 *                         1.455 -> 1.421 ms, 8 bounces 1.856 -> 1.819); 0: never;
 *                         1: always.  ptrt_get_option "pm1_dense_roots_eff" says what the last frame did.
 *   pm1_full_leaf -1|0|1  PMODE 1: when every leaf staged in LDS holds exactly as many triangles as the largest one (a scene of
 *                         cubes: 12 each), the triangle loops of the closest-hit and shadow traces leave out what only a shorter
 *                         leaf needs -- the count compare, the clamped slot, the address arithmetic per test -- and step one
 *                         pointer per pair.  The same tests in the same order: same bits.  -1 (default) and 1:
 *                         on when the leaves are uniform, decided on the host at upload; 0: never.  The batched ray queries
 *                         share the loops.  ptrt_get_option "pm1_full_leaf_eff" says what the last frame did (0 as well when
 *                         the leaves differ or another traversal mode rendered it).
 *   pm1_lane_groups -1|0|1   PMODE 1 with pm1_full_leaf in effect: the last, partial batch of a trace's pair list (n < 64 pairs)
 *                         gives every pair g lanes with g a DIVISOR of the leaf size -- 1, 2, 3, 4, 6 or 12 for cubes, where the
 *                         2^sh rule had 1, 2, 4 and, in the guarded loop, 8 -- and may run as several sub-batches (40 pairs: 32
 *                         at 2 lanes and 8 at 6, 6 + 2 test iterations for 12), by a plan the host makes at upload from the leaf
 *                         size (ptrt_pm1_plan).  The same (ray, triangle) tests and merges: same bits.  -1
 *                         (default) and 1: on when pm1_full_leaf is; 0: the 2^sh rule.  Closest-hit traces of a scene with an
 *                         instanced mesh keep one lane per pair.  The batched ray queries share the loops.  ptrt_get_option
 *                         "pm1_lane_groups_eff" says what the last frame or ray query did.
 *   plain_leaf -1|0|1     PMODE 1 and 2 (the traversals that build their (ray, mesh) pair lists with build_pairs over a single-leaf
 *                         TLAS; PMODE 4 builds its merged list with root tests of its own and does not read it): when no mesh of
 *                         the leaf has a transform and every mesh's root box lies inside the TLAS root box (fp32, component by
 *                         component; derived by ptrt_upload_geometry, ptrt_plain_leaf says it without a device), the pair
 *                         builder leaves out the TLAS root-box test -- a ray that misses the root passes no mesh's test, the slab
 *                         arithmetic is monotone -- and PMODE 1's pair batches the instance flag test and the t / dirScale
 *                         quotient of the merge.  Same pair list, same bits.  -1 (default) and 1: on where the
 *                         upload derived it (1 never forces it); 0: never.  Whatever lets the device move a box or a transform
 *                         unseen by the host -- ptrt_refit, ptrt_build_bvh, ptrt_refit_tlas, ptrt_reorder_tlas,
 *                         ptrt_update_instances, ptrt_set_instance_transforms_device, ptrt_set_instance_poses_device -- turns it
 *                         off until the next ptrt_upload_geometry.  ptrt_get_option "plain_leaf_eff" says what the last frame or
 *                         query did (0 as well under another traversal mode, PMODE 4 among them).  The value travels with a
 *                         launch's arguments: a frame recorded into a caller's hipGraph keeps the value from when it was captured,
 *                         as it keeps pair_split and the transform flag -- record again after any of the calls above.
 *   tri_frames -1|0|1     PMODE 1's megakernel: the tangent frame (T, B) that turns a BSDF sample into world space is read from a
 *                         per-triangle table instead of being computed at every vertex.  On a mesh without a transform the shading
 *                         normal is the packet's geometric normal or its negation, so ptrt_upload_geometry stores, with the
 *                         normals, what orthoBasis returns for both (64 bytes per triangle); a lane loads the record of its
 *                         triangle and side.  Same bits: the record holds the function's own result.  -1 (default) and 1: on
 *                         while the upload's normals stand and no mesh of the scene has a transform (1 never forces it); 0:
 *                         never.  The calls that turn plain_leaf off turn this off too until the next ptrt_upload_geometry -- a
 *                         refit writes new normals and no frames, so a scene that refits every frame keeps computing them.
 *                         ptrt_get_option "tri_frames_eff" says what the last frame did.  Travels with a launch's arguments as
 *                         plain_leaf does.
 *   atlas_lanes -1|1|4|16|64   ptrt_atlas_texels: the lanes that share one triangle's texel range (a wave takes 64 / lanes leaf
 *                         slots at a time).  -1 (default): chosen on the host from atlas texels / faces of the mesh (DESIGN.md
 *                         3.28); anything else is PTRT_E_INVALID.  Same bytes under every value.  ptrt_get_option
 *                         "atlas_lanes_eff" says what the last ptrt_atlas_texels ran (0: none yet).
 *   atlas_filter_tile -1|0|1  ptrt_atlas_filter: 1 stages a workgroup's 16 x 16 texels and their halo of 2 * step -- guides and
 *                         colours -- in LDS wherever that fits, which is at steps 1, 2 and 4; 0 reads every tap with global loads
 *                         at every step; -1 (default): per step, whichever was measured faster.  Same bytes
 *                         under every value.  ptrt_get_option "atlas_filter_tile_eff" says how many passes of the last
 *                         ptrt_atlas_filter ran the LDS tile (-1: none yet).
 *   tile_run 0..64        the one-tile-per-workgroup kernels' workgroup -> tile map.  Consecutive workgroups go to the eight XCDs in
 *                         turn; with n > 0, of every 8 n consecutive tiles XCD x renders tiles [x n, (x + 1) n) -- neighbours,
 *                         whose rays walk the same part of the trees, share an L2 -- instead of every eighth tile.  8 (default):
 *                         the fluid frame 0.941 -> 0.913 ms with a quarter of its L2 misses, showcase 3.18 -> 3.14, at 4K 24.5 -> 24.1
 *                         (4 .. 32 are within one percent of each other from 720p to 4K); 0: tile k on workgroup k.
 *                         Same bits (a permutation of independent tiles).
 *   tlas_rounds 0|1       real TLAS: shadow rays take one TLAS leaf per fill of the pair list (what > 1024 meshes use) instead of all
 *   pm1_wg 0|1|2          PMODE 1: tiles per workgroup (1 default; 2: two tiles share the LDS copies, six waves per SIMD; 0: 2 if it fits)
 *   lds_pad 0..32768      spare bytes of LDS per workgroup: fewer waves per CU (A/B of the occupancy)
 *   wavefront 0|1, async_lanes 0|1, shade_min 1..64   the alternative loop shapes of DESIGN.md 3.9
 *   wf_sort 0|1|2|4       wavefront stages: the shade stage bins 1 / 2 / 4 groups of 256 consecutive paths by class (finished,
 *                         regenerating, miss, hit mesh x specular flag x roulette) in LDS before shading them -- active-path
 *                         sorting; same bits; measured slower than unsorted, default 0
 *   time_kernels 0|1      1 (default): two events around the trace kernel feed ptrt_kernel_ms_history / ptrt_last_kernel_ms
 *   time_launches 0|1     1: three events around every launch of a frame that is dealt to the auxiliary streams ("pipeline"), on the
 *                         stream the launch runs on: ptrt_launch_ms_history (default 0: six more driver calls per frame)
 *   tm_prio 0..3          lane refill's tonemap pass: |1 on a stream of the highest priority (hipStreamCreateWithPriority) forked from
 *                         and joined to its launch's stream, |2 its waves at s_setprio 3 (A/B: DESIGN.md 3.12)
 *   atrous_exp 0|1        denoiser: 1 = the a-trous luminance weight exp(-dl^2 / 2 sigma^2) through the hardware exponential (v_exp_f32), as
 *                         the reference's `__expf` (denoiser.cuh:731); 0 (default) = the deterministic exponential the oracle defines,
 *                         bit-exact.  Mode 1 is held to a stated tolerance against the oracle (tests/test_denoiser.py: per-pixel
 *                         relative L2 of the denoised HDR image <= 1e-5 (measured 3.9e-7), RGB8 within 1 LSB)
 *   denoiser_active, motion_vectors, use_graphs 0|1 */
int ptrt_set_option(ptrt_ctx *ctx, const char *name, long long value);
/* Reads an option back, and -- read-only -- what the last ptrt_render launched, so that a measurement can name the kernel it
 * timed: render_mode (0 megakernel, 1 wavefront stages, 2 asynchronous lanes), pmode (0 lock-step, 1 pairs over LDS-staged
 * triangles, 2 pair queue, 3 TLAS rounds, 4 merged queue), merged_eff (loop shape of that launch), merged_decided (0 while
 * merged = -1 is still sampling), launches.  ABI 5.  Also read-only (ABI 6): query_pmode, the traversal of the last
 * ptrt_query_rays / ptrt_trace_rays / ptrt_query_radiance / ptrt_query_probes / ptrt_query_irradiance / ptrt_query_direct / ptrt_query_bounce (-1 none yet), and stream, the hipStream_t the context enqueues on. */
int ptrt_get_option(ptrt_ctx *ctx, const char *name, long long *value);

/* The plan behind option "pm1_lane_groups" for leaves of `leaf_triangles` triangles, as ptrt_upload_geometry builds it; needs
 * no device and no context.  For a tail of n = 1 .. 63 pairs, element n - 1 of out_g63 / out_take63 holds the first
 * sub-batch: g lanes per pair (a divisor of the leaf size; 0: this tail keeps the 2^sh rule's single batch, which then takes
 * all n) and the pairs it takes, min(n, 64 / g); the rest of the tail follows its own entry.  Optional (may be NULL): out_mul63,
 * the constant m with lane / g == (lane * m) >> 12 for lanes 0 .. 63; out_cost63, the whole tail's cost in the model's
 * wave-instructions; out_model2, the model {one test, one sub-batch header}.  Returns 1, 0 when the leaf size is outside the
 * plan's range (every tail keeps the 2^sh rule), -1 for a bad argument.  ptrt_pm1_div_mul: that m for g = 1 .. 64 (0
 * outside).  ABI 6, additions only. */
int ptrt_pm1_plan(int leaf_triangles, int32_t *out_g63, int32_t *out_take63, int32_t *out_mul63, int32_t *out_cost63,
                  int32_t *out_model2);
int ptrt_pm1_div_mul(int g);

/* What ptrt_upload_geometry derives for option "plain_leaf" from the same arrays; needs no device and no context.  1: the TLAS
 * root is a single leaf, no mesh of it has a transform, and node 0's box of every mesh of the leaf lies inside the TLAS root
 * box (fp32 compares, a NaN fails); 0: not so; -1: a missing array.  ABI 6, additions only. */
int ptrt_plain_leaf(const ptrt_mesh_desc *meshes, int mesh_count, const ptrt_bvh_node *tlas_nodes, int tlas_node_count,
                    const int32_t *tlas_mesh_indices, int tlas_index_count);

/* The dynamic LDS of a launch shape as the device carves it and the host counts it (csrc/lds_layout.h; DESIGN.md 2, "LDS
 * layouts"); needs no device and no context.  `shape`: a one-wave pair workgroup in PMODE 1 (as the device queries use it), 2,
 * 3 or 4; the PMODE 1 megakernel's workgroup of one or two waves, with what it stages from the budget of the occupancy its
 * kernel is built for; PMODE 2 in four-wave workgroups (option lds_nodes); the lock-step stacks of PMODE 0 (`stack_entries`
 * as launched: 0 where every BLAS is one leaf); the asynchronous-lane kernel; the wavefront trace stage.  A shape reads the
 * parameters it depends on and ignores the others.  Writes the regions in use -- at most max_regions of them -- one record per
 * region and wave (wave -1: one copy per workgroup): byte offset from the workgroup's base, size, the alignment of what is
 * stored there, and for a region that BY DESIGN lies inside others the first and last region id of the span that holds it
 * (-1: none; all other regions are pairwise disjoint).  info: the launch's byte count (0: PMODE 1 over every budget), the
 * waves, the PMODE 1 decisions (KParams lds_flags / lds_extra / lds_wave / lds_wave_bytes, tiles per workgroup), PMODE 4's pair
 * capacity between its clamps, and the largest leaf whose (lane, triangle) tests the leaf-pair list holds.  Returns the number
 * of regions in use, -1 for a bad argument.  ptrt_lds_region_name: a region id's name (NULL outside).  ABI 6, additions only. */
enum {
    PTRT_LDS_LOCKSTEP = 0,
    PTRT_LDS_PAIR1 = 1,
    PTRT_LDS_PAIR2 = 2,
    PTRT_LDS_PAIR3 = 3,
    PTRT_LDS_PAIR4 = 4,
    PTRT_LDS_PM1_WG = 5,
    PTRT_LDS_NODES = 6,
    PTRT_LDS_ASYNC = 7,
    PTRT_LDS_WAVEFRONT = 8
};
typedef struct ptrt_lds_params {
    int32_t meshes, tri_slots;     /* meshes of the single TLAS leaf; triangle slots staged (PMODE 1) */
    int32_t stack_entries;         /* BLAS stack entries per lane */
    int32_t tlas_leaf, tlas_depth; /* PMODE 3: largest TLAS leaf, TLAS stack entries per lane */
    int32_t lights;
    int32_t full, stage, lds_pad, pm1_wg, sample_sync; /* PMODE 1 megakernel: full materials, options stage / lds_pad / pm1_wg, samples in step */
} ptrt_lds_params;
typedef struct ptrt_lds_region {
    int32_t id, wave;
    int64_t offset, bytes;
    int32_t align, in_first, in_last;
} ptrt_lds_region;
typedef struct ptrt_lds_info {
    int64_t total;
    int32_t waves;
    int32_t lds_flags, lds_extra, lds_wave, lds_wave_bytes, wg;
    int32_t pair_cap, pair_cap_lo, pair_cap_hi;
    int32_t max_leaf;
} ptrt_lds_info;
int ptrt_lds_layout(int shape, const ptrt_lds_params *params, ptrt_lds_region *regions, int max_regions, ptrt_lds_info *info);
const char *ptrt_lds_region_name(int id);

/* Render on a caller-owned HIP stream (a `hipStream_t` passed as void*; NULL returns to the
 * context's own stream).  Lets a host that already orders work on a stream (a GL-interop map,
 * an RCCL gather) enqueue frames without host synchronisation, like the reference's use of
 * the default stream (SURVEY 8(b) "Threading / streams"). */
int ptrt_set_stream(ptrt_ctx *ctx, void *hip_stream);

/* Durations (ms) of the most recent path-trace kernel launches, oldest first, measured with
 * HIP events on the stream the kernel ran on; at most 256 are kept.  Synchronises.  Returns
 * the number written (<= max_n) or a negative error.  A launch's duration is asked of the runtime
 * once and kept (here, in ptrt_last_kernel_ms and in ptrt_launch_ms_history): the same launch reads
 * the same float every time, whatever ran in between. */
int ptrt_kernel_ms_history(ptrt_ctx *ctx, float *out_ms, int max_n);

/* Frames that overlap on the device (option "pipeline") run as `split` launches on auxiliary streams; the events of
 * ptrt_kernel_ms_history then bracket the frame INTERVAL on the context's stream.  With option "time_launches" on, this returns
 * the durations of the launches themselves, oldest first, over the unbroken run of such frames that ends with the last
 * ptrt_render: trace_ms[k] = the path-trace kernel of launch k (HIP events on the stream it ran on), tail_ms[k] (may be NULL) =
 * from its end to the end of the tonemap pass that follows it with lane refill (0 otherwise).  A frame contributes `split`
 * entries.  Synchronises.  Returns the number written (<= max_n) or a negative error.  No counterpart in the reference (it
 * times nothing); what bench.py's `roofline.kernel_ms` is measured with.  ABI 6. */
int ptrt_launch_ms_history(ptrt_ctx *ctx, float *trace_ms, float *tail_ms, int max_n);

/* duration in milliseconds of the last ptrt_render's path-trace kernel and
 * tonemap kernel, measured with HIP events on the context's stream
 * (synchronises).  Either pointer may be NULL. */
int ptrt_last_kernel_ms(ptrt_ctx *ctx, float *trace_ms, float *tonemap_ms);


/* ---- the one-bounce ray tracer of src/raytracer/ (RTscene.cuh, RTmesh.cuh, RTcamera.cuh) ---------------------------
 * A context of its own, separate from ptrt_ctx: the RT Scene keeps one geometry buffer and one BVH per mesh (no TLAS),
 * a descriptor array (material + rigid transform per mesh) and a light array, and renders render_kernel
 * (RTscene.cuh:1240-1293) into an RGB8 frame, bottom-up.  Every entry returns PTRT_OK or a negative code; the message,
 * naming the entry point, is read with ptrt_rt_last_error.  (ABI 6, additions only.) */
typedef struct ptrt_rt_ctx ptrt_rt_ctx;

typedef struct ptrt_rt_material { /* Material, RTscene.cuh:21-61 (108 B) */
    ptrt_vec3 albedo, specular;
    float metallic, roughness;
    ptrt_vec3 emission;
    float ior, transmission, transmission_roughness, clearcoat, clearcoat_roughness;
    ptrt_vec3 subsurface_color;
    float subsurface_radius, anisotropy, sheen;
    ptrt_vec3 sheen_tint;
    float iridescence, iridescence_thickness;
} ptrt_rt_material;

typedef struct ptrt_rt_mesh { /* the per-mesh part of DeviceMesh (RTscene.cuh:84-102): material and rigid transform */
    ptrt_rt_material material;
    ptrt_vec3 translation;
    float rotation[9], inv_rotation[9]; /* row-major mat3: rotY * rotX * rotZ and its transpose */
} ptrt_rt_mesh;

typedef struct ptrt_rt_light { /* Light, RTscene.cuh:64-80 (56 B): type 0 point, 1 directional, 2 spot; cones are cosines */
    int32_t type;
    ptrt_vec3 position, direction, color;
    float intensity, range, inner_cone, outer_cone;
} ptrt_rt_light;

typedef struct ptrt_rt_view { /* what render_kernel takes besides the arrays: Camera's vectors, ambient, sky */
    ptrt_vec3 origin, corner_minus_origin, horizontal, vertical;
    ptrt_vec3 ambient, sky_top, sky_bottom;
    int32_t use_sky;
} ptrt_rt_view;

/* Scene::Scene(w, h) of RTscene.cuh:789-796: a width x height frame on HIP device `device`.  PTRT_E_NO_DEVICE without
 * one (there is no CPU path). */
int ptrt_rt_create(int width, int height, int device, ptrt_rt_ctx **out);
/* Scene::~Scene (RTscene.cuh:798-808).  NULL and dead handles are ignored. */
void ptrt_rt_destroy(ptrt_rt_ctx *ctx);
/* The message of the context's last failure (of the thread's last failure for NULL or a dead handle). */
const char *ptrt_rt_last_error(const ptrt_rt_ctx *ctx);
/* Mesh::upload (RTmesh.cuh:420-431) of mesh slot `index` (< the slot count replaces, == appends): its vertices and
 * index triples, every index inside 0..vert_count-1.  The slot's BVH is kept: a tree uploaded earlier is walked over
 * the new triangles, as in the reference when vertices change without bvhDirty. */
int ptrt_rt_upload_mesh(ptrt_rt_ctx *ctx, int index, const ptrt_vec3 *verts, int vert_count, const ptrt_tri *faces,
                        int face_count);
/* Mesh::uploadBVH (RTmesh.cuh:554-568) of an existing slot: DeviceBVHNode array (node 0 the root, an inner node's
 * children -1 or after it, a leaf's range inside the primitive array) and the face indices of the leaves. */
int ptrt_rt_upload_bvh(ptrt_rt_ctx *ctx, int index, const ptrt_bvh_node *nodes, int node_count, const int32_t *prims,
                       int prim_count);
/* The descriptor part of Scene::uploadToGPU / render_to_device (RTscene.cuh:1031-1100, 1134-1196): material and
 * transform of slots 0..mesh_count-1 and the lights.  Copies descriptors only; geometry stays where it is. */
int ptrt_rt_set_scene(ptrt_rt_ctx *ctx, const ptrt_rt_mesh *meshes, int mesh_count, const ptrt_rt_light *lights,
                      int light_count);
/* The launch of Scene::render / render_to_device (RTscene.cuh:1102-1132, 1198-1210): render_kernel over the frame with
 * the last ptrt_rt_set_scene, into out_rgb8 (PTRT_OUT_HOST: host memory, PTRT_OUT_DEVICE: device memory of the
 * context's device, width*height*3 bytes each).  Synchronous, like the reference's cudaDeviceSynchronize.
 * PTRT_E_NOT_READY before ptrt_rt_set_scene; PTRT_E_INVALID if a mesh's tree names a face its geometry lacks. */
int ptrt_rt_render(ptrt_rt_ctx *ctx, const ptrt_rt_view *view, void *out_rgb8, int out_is_device);

#ifdef __cplusplus
}
#endif
#endif /* PTRT_H */
