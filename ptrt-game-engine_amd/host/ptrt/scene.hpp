// ptrt/scene.hpp -- the host API of the PTRT path tracer, over the MI355X back end.
//
// `class Scene` keeps the reference's method names, defaults and error behaviour
// (reference: src/pathtracer/scene/scene.cuh:78-2001) so a caller of the CUDA
// renderer can switch headers.  What differs is underneath: the scene is
// flattened once per change into plain arrays and handed to the C ABI of
// include/ptrt.h, which owns every device allocation.  Out of scope here (see
// DESIGN.md): the debug-visualisation helper meshes (frustum, ray arrows) -- their
// setters are accepted and recorded so call sites compile, and
// `updateVisualizationMeshes` reports when one is enabled.
#pragma once
#include "hdr.hpp"
#include "mesh.hpp"

#include <chrono>
#include <cstdint>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

// ---- Material (scene/material_lib.cuh:12-105) -----------------------------------------
struct Material {
    vec3 albedo{0.8f}, specular{0.04f};
    float metallic = 0.0f, roughness = 0.5f;
    vec3 emission{0.0f};
    float ior = 1.5f, transmission = 0.0f, transmissionRoughness = 0.0f;
    float clearcoat = 0.0f, clearcoatRoughness = 0.03f;
    vec3 subsurfaceColor{1.0f};
    float subsurfaceRadius = 0.0f, anisotropy = 0.0f, sheen = 0.0f;
    vec3 sheenTint{0.5f};
    float iridescence = 0.0f, iridescenceThickness = 550.0f;
    Material() = default;
    Material(const vec3 &alb, float rough = 0.5f, float met = 0.0f) {
        albedo = alb;
        roughness = rough;
        metallic = met;
        specular = lerp(vec3(0.04f), albedo, metallic);
        transmissionRoughness = fmaxf(transmissionRoughness, roughness);
    }
};

// conversion helpers of material_lib.cuh:128-146, used by the applications' material libraries (app_utils.cuh:79-103)
inline float phongShininessToRoughness(float n) {
    const float alpha = sqrtf(2.0f / (fmaxf(n, 1.0f) + 2.0f));
    return fminf(fmaxf(fmaxf(alpha, 0.02f), 0.0f), 1.0f);
}
inline float iorToF0(float ior) {
    const float a = (ior - 1.0f) / (ior + 1.0f);
    return a * a;
}

// ---- Light (scene/lights.cuh) ---------------------------------------------------------
enum LightType { LIGHT_POINT = 0, LIGHT_DIRECTIONAL = 1, LIGHT_SPOT = 2 };
struct Light {
    LightType type = LIGHT_POINT;
    vec3 position{0, 10, 0}, direction{0, -1, 0}, color{1.0f};
    float intensity = 1.0f, range = 100.0f, innerCone = 0.5f, outerCone = 0.7f, radius = 0.0f;
};

// ---- Camera (scene/camera.cuh:32-205, ray-generation state only) ----------------------
class Camera {
    vec3 origin, lower_left_corner, horizontal, vertical, u, v, w;
    float lens_radius = 0.0f, fov = 90.0f, aspect = 1.0f, near_clip = 0.1f, far_clip = 1000.0f;
    mat4 view_matrix, proj_matrix; // for motion vectors (camera.cuh:41-43,88-95)

    void update_matrices(const vec3 &lookfrom, const vec3 &lookat, const vec3 &vup) {
        view_matrix = mat4::lookAt(lookfrom, lookat, vup);
        proj_matrix = mat4::perspective(fov * (PI / 180.0f), aspect, near_clip, far_clip);
    }
    void rebuild(const vec3 &lookat, const vec3 &vup, float focus_dist) {
        update_matrices(origin, lookat, vup);
        w = (origin - lookat).normalized();
        u = cross(vup, w).normalized();
        v = cross(w, u);
        const float theta = fov * (PI / 180.0f);
        const float h = tanf(theta / 2.0f);
        const float viewport_height = 2.0f * h;
        const float viewport_width = aspect * viewport_height;
        horizontal = focus_dist * viewport_width * u;
        vertical = focus_dist * viewport_height * v;
        lower_left_corner = origin - horizontal * 0.5f - vertical * 0.5f - focus_dist * w;
    }

  public:
    Camera(vec3 lookfrom, vec3 lookat, vec3 vup, float vfov, float aspect_ratio, float aperture = 0.0f,
           float focus_dist = 1.0f, float znear = 0.1f, float zfar = 1000.0f) {
        origin = lookfrom;
        fov = vfov;
        aspect = aspect_ratio;
        near_clip = znear;
        far_clip = zfar;
        rebuild(lookat, vup, focus_dist);
        lens_radius = aperture / 2.0f;
    }
    explicit Camera(float aspect_ratio, float viewport_height = 2.0f, float focal_length = 1.0f) {
        origin = vec3(0.0f);
        const float viewport_width = viewport_height * aspect_ratio;
        horizontal = vec3(viewport_width, 0.0f, 0.0f);
        vertical = vec3(0.0f, viewport_height, 0.0f);
        lower_left_corner = origin - horizontal * 0.5f - vertical * 0.5f - vec3(0.0f, 0.0f, focal_length);
        u = vec3(1, 0, 0);
        v = vec3(0, 1, 0);
        w = vec3(0, 0, 1);
        aspect = aspect_ratio;
        fov = 90.0f;
        near_clip = 0.1f;
        far_clip = 100.0f;
        update_matrices(origin, vec3(0, 0, -1), vec3(0, 1, 0));
    }
    mat4 get_view_proj() const { return proj_matrix * view_matrix; } // camera.cuh:257-259
    // get_ray_simple (camera.cuh:201-205); the debug-ray helper is the only host caller
    void get_ray(float s, float t, vec3 &o, vec3 &d) const {
        o = origin;
        d = (lower_left_corner + s * horizontal + t * vertical - origin).normalized();
    }
    vec3 get_origin() const { return origin; }
    vec3 get_lower_left_corner() const { return lower_left_corner; }
    vec3 get_horizontal() const { return horizontal; }
    vec3 get_vertical() const { return vertical; }
    void set_position(const vec3 &pos) { // camera.cuh:271-299
        vec3 old_center = lower_left_corner + 0.5f * horizontal + 0.5f * vertical;
        float focus_dist = (origin - old_center).length();
        vec3 lookat = origin - w * focus_dist;
        vec3 vup = v;
        origin = pos;
        rebuild(lookat, vup, (origin - lookat).length());
    }
    void look_at(const vec3 &target, const vec3 &vup = vec3(0, 1, 0)) { // camera.cuh:306-331
        rebuild(target, vup, (origin - target).length());
    }
    ptrt_camera flat() const {
        auto c = [](const vec3 &a) { return ptrt_vec3{a.x, a.y, a.z}; };
        return ptrt_camera{c(origin), c(lower_left_corner), c(horizontal), c(vertical), c(u), c(v), c(w), lens_radius};
    }
};

// ---- blue-noise table (common/bluenoise.cuh:79-198) -----------------------------------
// 64x64 jittered-stratified points relaxed by 25 rounds of O(N^2) toroidal
// repulsion.  std::uniform_real_distribution<float> is implementation-defined;
// the table this produces with libstdc++ is pinned in tests/golden/.
struct BlueNoiseGenerator {
    static std::vector<float> generateBlueNoise2D(int size, int relaxation_iterations) {
        const int n = size * size;
        std::vector<float> px(n), py(n), fx(n), fy(n);
        std::mt19937 rng(12345);
        std::uniform_real_distribution<float> dist(0.0f, 1.0f);
        const float cell = 1.0f / size;
        for (int y = 0; y < size; ++y)
            for (int x = 0; x < size; ++x) {
                const float jx = dist(rng); // x first, then y, one pair per point
                const float jy = dist(rng);
                px[y * size + x] = (x + jx) * cell;
                py[y * size + x] = (y + jy) * cell;
            }
        const float step = 0.0001f, min_d2 = 0.0001f;
        auto wrap = [](float a) {
            float r = std::fmod(a, 1.0f);
            return r < 0.0f ? r + 1.0f : r;
        };
        for (int it = 0; it < relaxation_iterations; ++it) {
            for (int i = 0; i < n; ++i) {
                float ax = 0.0f, ay = 0.0f;
                const float xi = px[i], yi = py[i];
                for (int j = 0; j < n; ++j) {
                    if (i == j)
                        continue;
                    float dx = xi - px[j], dy = yi - py[j];
                    if (dx > 0.5f) dx -= 1.0f;
                    if (dx < -0.5f) dx += 1.0f;
                    if (dy > 0.5f) dy -= 1.0f;
                    if (dy < -0.5f) dy += 1.0f;
                    float d2 = dx * dx + dy * dy;
                    d2 = std::max(d2, min_d2);
                    const float inv = 1.0f / d2;
                    ax += dx * inv;
                    ay += dy * inv;
                }
                fx[i] = ax;
                fy[i] = ay;
            }
            for (int i = 0; i < n; ++i) {
                const float mag = std::sqrt(fx[i] * fx[i] + fy[i] * fy[i]);
                if (mag < 1e-6f)
                    continue;
                px[i] = wrap(px[i] + (fx[i] / mag) * step);
                py[i] = wrap(py[i] + (fy[i] / mag) * step);
            }
        }
        std::vector<float> out((size_t)n * 2);
        for (int i = 0; i < n; ++i) {
            out[i * 2] = px[i];
            out[i * 2 + 1] = py[i];
        }
        return out;
    }
};
// the table initBlueNoise() would upload (bluenoise.cuh:189-198), computed once per process
inline const std::vector<float> &ptrtBlueNoiseTable() {
    static const std::vector<float> t = BlueNoiseGenerator::generateBlueNoise2D(PTRT_BLUE_NOISE_SIZE, 25);
    return t;
}

struct HitInfo { // math/intersection.cuh:108-124
    bool hit = false;
    float t = 1e30f;
    vec3 point, normal;
    int mesh_index = -1;
    bool front_face = true;
    float u = 0, v = 0;
    int face_index = -1;
    vec3 localPoint;
};

// ---- Scene ----------------------------------------------------------------------------
// device of `Scene(w, h)`; -1 = host-only scenes (build / flatten / inspect on a box without a GPU)
#ifndef PTRT_DEFAULT_DEVICE
#define PTRT_DEFAULT_DEVICE 0
#endif
class Scene {
  public:
    struct PerformanceSettings { // scene.cuh:189-199
        bool enableDenoiser = true;
        bool enableBloom = true;
        bool enableMotionVectors = true;
        int maxBounceDepth = 4;
        int samplesPerPixel = 1;
        float resolutionScale = 1.0f;
        bool fastBVHUpdates = true;          // never read by the reference either
        bool enableRussianRoulette = true;   // never read: RR always starts at bounce 2
        int russianRouletteStartBounce = 1;  // never read (path_logic.cuh:24)
    };

    // Scene(w,h) of the reference; the extra arguments select a band of rows and a
    // device for tile-parallel rendering and default to "whole frame,
    // device 0".
    Scene(int w, int h, int tile_y0 = 0, int tile_rows = 0, int device = PTRT_DEFAULT_DEVICE)
        : width(w), height(h), camera(static_cast<float>(w) / h, 2.0f, 1.0f) {
        tileRows = tile_rows > 0 ? tile_rows : h;
        tileY0 = tile_y0;
        device_ = device;
        render_width = w;
        render_height = h;
        if (device < 0)
            return; // host-only scene: build/flatten/inspect, no back end (every GPU call then fails loudly)
        int rc = ptrt_create(w, h, tile_y0, tile_rows, device, &ctx);
        if (rc != PTRT_OK) {
            std::string msg = std::string("Failed to create GPU context: ") + ptrt_last_error(ctx);
            ptrt_destroy(ctx);
            ctx = nullptr;
            throw std::runtime_error(msg);
        }
        try { // a constructor that throws never runs ~Scene: the context must not outlive it
            check(ptrt_reset_rng(ctx, PTRT_DEFAULT_SEED), "Failed to init rand states"); // scene.cuh:433-456
            if (tileRows == h && tile_y0 == 0) {
                // `denoiser_ = new Denoiser(settings)` (scene.cuh:1984-1993): exists from construction,
                // used while perfSettings.enableDenoiser; band contexts cannot denoise (filters cross bands)
                fullFrame = true;
                check(ptrt_denoiser_enable(ctx, nullptr), "Failed to create denoiser");
                denoiserAllocated = true;
            }
        } catch (...) {
            ptrt_destroy(ctx);
            ctx = nullptr;
            throw;
        }
        prev_view_proj = camera.get_view_proj();
    }
    // Tile farm, second way of cutting the frame: this scene renders every `period`-th 8-row strip starting with
    // strip `phase` (ptrt_create_interleaved).  No post chain, like a band.
    struct Interleave {
        int phase, period;
    };
    Scene(int w, int h, Interleave il, int device = PTRT_DEFAULT_DEVICE)
        : width(w), height(h), camera(static_cast<float>(w) / h, 2.0f, 1.0f) {
        tileY0 = il.phase * 8;
        device_ = device;
        render_width = w;
        render_height = h;
        tileRows = 0;
        for (int t = il.phase; t * 8 < h; t += (il.period < 1 ? 1 : il.period))
            tileRows += (t * 8 + 8 <= h) ? 8 : h - t * 8;
        if (device < 0)
            return;
        if (ptrt_create_interleaved(w, h, il.phase, il.period, device, &ctx) != PTRT_OK) {
            std::string msg = std::string("Failed to create GPU context: ") + ptrt_last_error(ctx);
            ptrt_destroy(ctx);
            ctx = nullptr;
            throw std::runtime_error(msg);
        }
        try {
            check(ptrt_reset_rng(ctx, PTRT_DEFAULT_SEED), "Failed to init rand states");
        } catch (...) {
            ptrt_destroy(ctx);
            ctx = nullptr;
            throw;
        }
        prev_view_proj = camera.get_view_proj();
    }
    ~Scene() { ptrt_destroy(ctx); }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    // the application's `initBlueNoise()` call; without it the table is all zeros,
    // exactly as in the reference (bluenoise.cuh:46,189)
    void initBlueNoise() { needBackend(); check(ptrt_set_blue_noise(ctx, ptrtBlueNoiseTable().data()), "blue noise upload failed"); }
    void setBlueNoiseTable(const float *table) { needBackend(); check(ptrt_set_blue_noise(ctx, table), "blue noise upload failed"); }

    // ---- accumulation / acceleration settings (scene.cuh:1270-1296) -----------------
    void resetAccumulation() {
        frame_count_ = 0;
        prev_view_proj = camera.get_view_proj(); // scene.cuh:1282: no motion across a reset
    }
    void setBVHLeafTarget(int target, int tol = 5) {
        bvhLeafTarget_ = target < 1 ? 1 : target;
        bvhLeafTol_ = tol < 0 ? 0 : tol;
        for (auto &m : meshes)
            m->bvhDirty = true;
        resetAccumulation();
    }

    // ---- camera (scene.cuh:1298-1331) -----------------------------------------------
    void setCamera(const vec3 &lookfrom, const vec3 &lookat, const vec3 &vup, float vfov, float aperture = 0.0f,
                   float focus_dist = 1.0f) {
        camera = Camera(lookfrom, lookat, vup, vfov, static_cast<float>(width) / height, aperture, focus_dist);
        cameraDirty = true;
        resetAccumulation();
    }
    void setCameraSimple(float viewport_height = 2.0f, float focal_length = 1.0f) {
        camera = Camera(static_cast<float>(width) / height, viewport_height, focal_length);
        cameraDirty = true;
        resetAccumulation();
    }
    vec3 cameraOrigin() const { return camera.get_origin(); }
    vec3 cameraForward() const {
        return (camera.get_lower_left_corner() + camera.get_horizontal() * 0.5f + camera.get_vertical() * 0.5f -
                camera.get_origin())
            .normalized();
    }
    void moveCamera(const vec3 &pos) { camera.set_position(pos); cameraDirty = true; resetAccumulation(); }
    void lookCameraAt(const vec3 &target, const vec3 &vup = vec3(0, 1, 0)) {
        camera.look_at(target, vup);
        cameraDirty = true;
        resetAccumulation();
    }
    Camera &getCamera() { cameraDirty = true; return camera; }

    // ---- geometry (scene.cuh:1334-1500) ---------------------------------------------
    Mesh *addMesh(const std::string &obj_path, const Material &mat = Material()) {
        return push(std::make_unique<Mesh>(obj_path), mat);
    }
    Mesh *addTriangles(const std::vector<Triangle> &tris, const Material &mat = Material()) {
        auto m = std::make_unique<Mesh>();
        m->vertices.clear();
        m->faces.clear();
        m->vertices.reserve(tris.size() * 3);
        m->faces.reserve(tris.size());
        for (const Triangle &t : tris) {
            const int base = (int)m->vertices.size();
            m->vertices.push_back(t.v0);
            m->vertices.push_back(t.v1);
            m->vertices.push_back(t.v2);
            m->faces.push_back(Tri{base, base + 1, base + 2});
        }
        return push(std::move(m), mat);
    }
    Mesh *addPlaneXZ(float planeY, float halfSize, const Material &mat = Material(vec3(0.8f))) {
        const vec3 A(-halfSize, planeY, -halfSize), B(halfSize, planeY, -halfSize), C(halfSize, planeY, halfSize),
            D(-halfSize, planeY, halfSize);
        return addTriangles({Triangle(A, C, B), Triangle(A, D, C)}, mat); // CCW from +Y
    }
    void addCheckerboardPlaneXZ(float planeY, int tilesPerSide, float tileSize, const Material &whiteMat,
                                const Material &blackMat) {
        std::vector<Triangle> white, black;
        const int N = tilesPerSide;
        const float start = -N * tileSize;
        for (int iz = 0; iz < 2 * N; ++iz)
            for (int ix = 0; ix < 2 * N; ++ix) {
                const float x0 = start + ix * tileSize, x1 = x0 + tileSize;
                const float z0 = start + iz * tileSize, z1 = z0 + tileSize;
                const vec3 A(x0, planeY, z0), B(x1, planeY, z0), C(x1, planeY, z1), D(x0, planeY, z1);
                auto &bucket = (((ix + iz) & 1) == 0) ? white : black;
                bucket.emplace_back(A, C, B);
                bucket.emplace_back(A, D, C);
            }
        if (!white.empty())
            addTriangles(white, whiteMat);
        if (!black.empty())
            addTriangles(black, blackMat);
    }
    Mesh *addCube(const Material &mat = Material(vec3(1.0f, 0.0f, 0.0f))) { return push(std::make_unique<Mesh>(), mat); }
    // UV sphere of diameter 1: (segments+1)^2 vertices, 2*segments^2 faces (scene.cuh:1455-1500)
    Mesh *addSphere(int segments = 32, const Material &mat = Material(vec3(1.0f, 0.0f, 0.0f))) {
        auto m = std::make_unique<Mesh>();
        m->vertices.clear();
        m->faces.clear();
        const int rings = segments, sectors = segments;
        const float radius = 0.5f;
        for (int r = 0; r <= rings; ++r) {
            const float phi = PI * float(r) / float(rings);
            const float y = cosf(phi) * radius;
            const float ringRadius = sinf(phi) * radius;
            for (int s = 0; s <= sectors; ++s) {
                const float theta = TWO_PI * float(s) / float(sectors);
                m->vertices.push_back(vec3(ringRadius * cosf(theta), y, ringRadius * sinf(theta)));
            }
        }
        for (int r = 0; r < rings; ++r)
            for (int s = 0; s < sectors; ++s) {
                const int curr = r * (sectors + 1) + s, next = curr + sectors + 1;
                m->faces.push_back({curr, next, curr + 1});
                m->faces.push_back({curr + 1, next, next + 1});
            }
        return push(std::move(m), mat);
    }

    // ---- lights (scene.cuh:1503-1545, 1800-1827) -------------------------------------
    void addPointLight(const vec3 &position, const vec3 &color, float intensity = 1.0f, float range = 100.0f,
                       float radius = 0.0f) {
        Light l;
        l.type = LIGHT_POINT;
        l.position = position;
        l.color = color;
        l.intensity = intensity;
        l.range = range;
        l.radius = radius;
        addLight(l);
    }
    void addDirectionalLight(const vec3 &direction, const vec3 &color, float intensity = 1.0f) {
        Light l;
        l.type = LIGHT_DIRECTIONAL;
        l.direction = direction.normalized();
        l.color = color;
        l.intensity = intensity;
        addLight(l);
    }
    // cone angles are given in radians and stored as cosines
    void addSpotLight(const vec3 &position, const vec3 &direction, const vec3 &color, float intensity = 1.0f,
                      float innerCone = 0.5f, float outerCone = 0.7f, float range = 100.0f, float radius = 0.0f) {
        Light l;
        l.type = LIGHT_SPOT;
        l.position = position;
        l.direction = direction.normalized();
        l.color = color;
        l.intensity = intensity;
        l.innerCone = cosf(innerCone);
        l.outerCone = cosf(outerCone);
        l.range = range;
        l.radius = radius;
        addLight(l);
    }
    Light *getLight(size_t i) { return i < lights.size() ? &lights[i] : nullptr; }
    size_t getLightCount() const { return lights.size(); }
    void moveLightTo(size_t i, const vec3 &position) {
        if (Light *l = getLight(i)) {
            l->position = position;
            lightsDirty = true;
            resetAccumulation();
        }
    }
    void commitLightChanges() {
        if (!lights.empty()) {
            lightsDirty = true;
            resetAccumulation();
        }
    }

    // ---- sky (scene.cuh:1548-1565) ---------------------------------------------------
    void setSkyGradient(const vec3 &top, const vec3 &bottom) {
        sky_color_top = top;
        sky_color_bottom = bottom;
        use_sky = true;
        skyDirty = true;
        resetAccumulation();
    }
    void disableSky() { use_sky = false; skyDirty = true; resetAccumulation(); }
    // scene.cuh:958-1026: an equirectangular .hdr picture becomes the sky (stbi_loadf, 4 channels,
    // flipped vertically -> host/ptrt/hdr.hpp reads the same floats); sampleSky then looks it up
    // instead of the gradient.  setEnvironmentMap is the same without the file.
    void loadHDRI(const std::string &filepath) {
        std::cout << "Loading HDRI: " << filepath << "..." << std::endl;
        std::vector<float> rgba;
        int w = 0, h = 0;
        ptrt_detail::load_radiance_hdr(filepath, w, h, rgba);
        std::cout << "Loaded HDRI: " << w << "x" << h << std::endl;
        setEnvironmentMap(rgba.data(), w, h);
    }
    void setEnvironmentMap(const float *rgba, int w, int h) {
        if (!rgba || w < 1 || h < 1)
            throw std::runtime_error("setEnvironmentMap: empty map");
        envMap.assign(rgba, rgba + (size_t)w * h * 4);
        env_width = w;
        env_height = h;
        envDirty = true;
        use_sky = true;
        skyDirty = true;
        resetAccumulation();
    }
    void freeHDRI() { // scene.cuh:944-956
        envMap.clear();
        env_width = env_height = 0;
        envDirty = true;
    }

    // ---- materials / objects ---------------------------------------------------------
    void setMeshMaterial(size_t index, const Material &mat) {
        if (index < mesh_materials.size())
            mesh_materials[index] = mat;
    }
    void commitMaterialChanges() { materialsDirty = true; resetAccumulation(); }
    Mesh *getMesh(size_t i) { return i < meshes.size() ? meshes[i].get() : nullptr; }
    const Mesh *getMesh(size_t i) const { return i < meshes.size() ? meshes[i].get() : nullptr; }
    size_t getMeshCount() const { return meshes.size(); }
    void moveMeshTo(size_t i, const vec3 &p) { if (Mesh *m = getMesh(i)) m->moveTo(p); }
    void translateMesh(size_t i, const vec3 &d) { if (Mesh *m = getMesh(i)) m->translate(d); }
    void rotateMesh(size_t i, const vec3 &r) { if (Mesh *m = getMesh(i)) m->rotateSelfEulerXYZ(r); }
    void scaleMesh(size_t i, float s) { if (Mesh *m = getMesh(i)) m->scale(s); }
    void scaleMesh(size_t i, const vec3 &s) { if (Mesh *m = getMesh(i)) m->scale(s); }
    void commitObjectChanges() { updateAccelerationStructures(); resetAccumulation(); } // scene.cuh:1784
    // What commitObjectChanges() / render_to_device() do with a mesh whose vertices were rewritten (bvhDirty / vertsDirty set
    // by the caller, as updatePTScene does for a `Triangles` mesh, PTRTtransfer.cuh:2249-2270, or by the vertex-baking
    // transforms) while its vertex count and face list are what was uploaded:
    //   HostRebuild (default) -- the reference: Mesh::buildBVH on the CPU, every mesh re-laid-out and re-uploaded
    //                            (scene.cuh:656-733);
    //   GpuRefit   -- the uploaded tree is kept: the new positions go to the device (ptrt_update_vertices) and the boxes are
    //                 refitted there (ptrt_refit); no host build, no re-upload of the arena;
    //   GpuRebuild -- as GpuRefit, but the faces are re-assigned to the leaves in Morton order first (ptrt_build_bvh).
    //   GpuRefitAll -- as GpuRefit, and a mesh whose instance transform changed goes through refitInstanceChanges(): the TLAS
    //                 is refitted on the device over the uploaded topology (ptrt_refit_tlas) and rebuilt nowhere; reseatTLAS()
    //                 gives it a fresh topology when the caller wants one.
    // A changed face list, vertex count, a new mesh, or a mesh without an uploaded tree falls back to HostRebuild for that
    // commit.  The host copy of a tree kept on the GPU is brought up to date when something reads it (flatten(), a real
    // TLAS, the next full upload).  So the UNCHANGED call sequence updatePTScene(scene, unified) -> commitObjectChanges()
    // reaches the GPU refit once the application has said  scene.setDynamicGeometryPolicy(...)  after building it.
    // Every entry point that edits geometry on the device -- this commit, refit* / rebuild* / updateTriangles below -- hands a
    // description of the edit to ONE route (editOnDevice), and what the device holds of a mesh, with whether the host copy of
    // its tree is current, is ONE record (Resident); DESIGN.md 3.4 has the table.
    enum class DynamicGeometryPolicy { HostRebuild = 0, GpuRefit = 1, GpuRebuild = 2, GpuRefitAll = 3 };
    void setDynamicGeometryPolicy(DynamicGeometryPolicy p) {
        dynPolicy = p;
        // (chosen after the upload: the face lists of the meshes nobody has touched since are what the device holds)
        if (p != DynamicGeometryPolicy::HostRebuild && gpu_resources_initialized && !geometryDirty && resident.size() == meshes.size())
            for (size_t i = 0; i < meshes.size(); ++i)
                if (resident[i].faces.empty() && !meshes[i]->bvhDirty && !meshes[i]->vertsDirty)
                    recordResident(i);
    }
    DynamicGeometryPolicy getDynamicGeometryPolicy() const { return dynPolicy; }
    // commits that took the GPU path / that re-uploaded the geometry (tests, bench)
    // host time (microseconds, accumulated) the mirror itself spends in a commit -- updateAccelerationStructures(): the
    // dynamic-geometry policy's topology check, the vertex hand-over, the refit / rebuild launches, the host structures --
    // and of that the part spent comparing face lists; for measurements (bench.py --via-commit), not part of the reference's API
    double commitHostMicros() const { return commitMicros; }
    double commitCompareMicros() const { return compareMicros; }
    size_t gpuDynamicCommitCount() const { return gpuDynamicCommits; }
    size_t geometryUploadCount() const { return geometryUploads; }
    // Dynamic geometry with unchanged topology (the fluid-sim caller, PTRTtransfer.cuh:2249-2270):
    // instead of commitObjectChanges()' full CPU rebuild, keep every tree and refit its boxes --
    // on the host copy (so flatten() stays consistent) and on the GPU (ptrt_update_vertices +
    // ptrt_refit, no re-upload of the arena).  Not in the reference.
    void refitObjectChanges() {
        requireUploaded("refitObjectChanges");
        editOnDevice(takeVertsDirty(), Trees::Refit, HostTrees::FollowNow, Tlas::RebuiltOnHost);
        resetAccumulation();
    }
    // TLAS over the meshes' new boxes: the host copy always; the device copy too when the TLAS has inner nodes
    // (the GPU refit moves the root box of a single-leaf TLAS itself and leaves a real TLAS to the host, which
    // rebuilds it as the reference's commit does)
    void syncTLAS() {
        buildTLAS();
        hostTlas = HostTlas::Current;
        pointFlatAtTLAS();
        if (h_tlasNodes.size() > 1)
            sendInstances("Failed to update the TLAS");
    }
    // same, the new positions already being in device memory (no host copy is kept: flatten()
    // then describes the LAST host-side vertices)
    void refitFromDevice(size_t mesh, const float *device_xyz) {
        editOnDevice({vertexEdit("refitFromDevice", mesh, device_xyz, true)}, Trees::Refit, HostTrees::LeftBehind, Tlas::RefittedOnDevice);
        resetAccumulation();
    }

    // same from HOST memory without touching the host copy of the mesh (its vertices are whatever the caller last put
    // there, and so is its tree): ptrt_update_vertices(on_device = 0) + ptrt_refit
    void refitFromHost(size_t mesh, const float *host_xyz) {
        editOnDevice({vertexEdit("refitFromHost", mesh, host_xyz, false)}, Trees::Refit, HostTrees::LeftBehind, Tlas::RefittedOnDevice);
        resetAccumulation();
    }

    // commitObjectChanges() for meshes whose face count is unchanged, with the BVH rebuilt ON THE GPU
    // (ptrt_build_bvh: Morton-order median split over the uploaded tree shape + refit) instead of
    // Mesh::buildBVH on the CPU + re-upload (scene.cuh:656-733).  The host copy of each rebuilt tree
    // follows (prim order read back, boxes refitted) so flatten() describes what the GPU traverses.
    // Without `syncHostCopy`, behind a TLAS with inner nodes the host copy follows lazily, as under the GpuRebuild policy: left
    // dirty, the mesh would be rebuilt on the host and everything uploaded again by the next frame, a second topology.
    void rebuildObjectChanges(bool syncHostCopy = true) {
        requireUploaded("rebuildObjectChanges");
        editOnDevice(takeVertsDirty(), Trees::Rebuild, syncHostCopy ? HostTrees::FollowNow : HostTrees::MarkedBehindInnerNodes,
                     syncHostCopy ? Tlas::RebuiltOnHost : Tlas::RefittedOnDevice);
        resetAccumulation();
    }
    // same, new positions already in device memory (host copy not updated)
    void rebuildFromDevice(size_t mesh, const float *device_xyz) {
        editOnDevice({vertexEdit("rebuildFromDevice", mesh, device_xyz, true)}, Trees::Rebuild, HostTrees::LeftBehind, Tlas::RefittedOnDevice);
        resetAccumulation();
    }
    // updatePTScene's `Triangles` path (PTRTtransfer.cuh:2204-2385) for a soup mesh made by
    // addTriangles with room for its original triangle count: `tri_count` new triangles (9 floats
    // each) from host or device memory, BVH rebuilt on the GPU.  The host copy of the mesh gets the
    // same padded vertices when the data is on the host; from device memory neither it nor any TLAS follows.
    void updateTriangles(size_t mesh, const float *verts9, int tri_count, bool on_device = false) {
        editOnDevice({vertexEdit("updateTriangles", mesh, verts9, on_device, tri_count)}, Trees::Rebuild,
                     on_device ? HostTrees::LeftBehind : HostTrees::FollowNow, on_device ? Tlas::Untouched : Tlas::RebuiltOnHost);
        resetAccumulation();
    }
    // Instances moved, nothing else changed, and the TLAS keeps the topology it was uploaded with (not in the reference, whose
    // commit rebuilds the TLAS on the CPU: scene.cuh:458-594, 656-743).  Every mesh whose transform is dirty or whose world
    // matrix differs from the last one handed over gets new matrices on the device -- one ptrt_set_instance_transforms per run
    // of consecutive meshes -- and ptrt_refit_tlas refits the TLAS there; nothing waits for the stream.  The host TLAS is
    // refitted over the same topology (refitTLAS), so flatten() describes what the GPU traverses.
    void refitInstanceChanges() {
        requireUploaded("refitInstanceChanges");
        refitMovedInstances();
        resetAccumulation();
    }
    // refitInstanceChanges() with a fresh ORDER first: moved instances' matrices go over, then ptrt_reorder_tlas re-deals the
    // meshes to the TLAS indices in Morton order of their world boxes' centres and refits (pt_tlas.hip.h) -- no upload, no
    // synchronisation.  The host TLAS follows through the same arithmetic (reorderTLASOnHost's), so flatten() describes what
    // the GPU traverses; where host root boxes lag the device's it follows by read-back when something reads it.
    void reorderTLAS() {
        requireUploaded("reorderTLAS");
        refitMovedInstances(true);
        resetAccumulation();
    }
    // (the work of refitInstanceChanges and reorderTLAS; a commit under GpuRefitAll comes here as well)
    void refitMovedInstances(bool reorder = false) {
        std::vector<ptrt_instance_xform> run; // (consecutive moved meshes [i - run.size(), i) awaiting one call)
        for (size_t i = 0; i <= meshes.size(); ++i) {
            if (i < meshes.size() && takeInstanceMove(i)) {
                run.emplace_back();
                writeInstance(run.back(), meshes[i]->transform);
            } else if (!run.empty()) {
                check(ptrt_set_instance_transforms(ctx, (int)(i - run.size()), (int)run.size(), run.data()), "Failed to set instance transforms");
                run.clear();
            }
        }
        if (reorder)
            check(ptrt_reorder_tlas(ctx), "Failed to re-order the TLAS");
        else
            check(ptrt_refit_tlas(ctx), "Failed to refit the TLAS");
        bool roots_lag = hostTlas != HostTlas::Current; // (host root boxes that lag the device's: the host TLAS follows by read-back, lazily)
        for (const Resident &r : resident)
            roots_lag = roots_lag || r.hostTree != HostTree::Current;
        if (roots_lag)
            markHostTlas(reorder && h_tlasNodes.size() > 1 ? HostTlas::OrderStale : HostTlas::BoxesStale);
        else
            refitHostTLAS(reorder);
    }
    // the host half alone, for a Scene without a back end (tests, tools that only flatten())
    void refitInstanceChangesOnHost() { moveInstancesOnHost("refitInstanceChangesOnHost", false); }
    // Host twin of ptrt_reorder_tlas, for a Scene without a back end as well: h_tlasMeshIndices in Morton order of the meshes'
    // world-box centres (mortonOrderTLAS), then refitTLAS() over the kept topology.
    void reorderTLASOnHost() { moveInstancesOnHost("reorderTLASOnHost", true); }
    // Host twin of ptrt_refit_tlas: the boxes of h_tlasNodes over the topology they have -- every mesh's world box from its
    // root box through Transform3D::transformAABB (as buildTLAS takes it), every leaf the union of its members, every inner
    // node the union of its children.  min / max are exact: the device's refit gives the same bits.
    void refitTLAS() { refitHostTLAS(false); }
    std::vector<AABB> meshWorldBoxes() const {
        if (h_tlasNodes.empty())
            throw std::runtime_error("refitTLAS: no TLAS built yet");
        std::vector<AABB> world(meshes.size());
        for (size_t i = 0; i < meshes.size(); ++i)
            world[i] = meshWorldBox(i);
        return world;
    }
    // pt::reorder_tlas_kernel on the host (morton30 / spread10 of csrc/pt_build.hip.h restated: change both or neither), operation by operation (-ffp-contract=off on both sides): mesh i's key is the
    // 30-bit Morton code of its world box's centre, (bmin + bmax) * 0.5f, within the bounds of all centres -- one scale, the
    // largest extent; t = (c - lo) / ext clamped to [0, 1]; min((int)(t * 1024), 1023) per axis, x in the high bit; ext == 0:
    // code 0 -- above the mesh index; TLAS index j gets the mesh ranked j.  The node array keeps its shape (the builder gives
    // a mesh count one shape); the caller refits its boxes.  A single-leaf TLAS keeps its order, as on the device.
    void mortonOrderTLAS(const std::vector<AABB> &world) {
        if (h_tlasNodes.size() <= 1)
            return;
        const size_t n = meshes.size();
        if (h_tlasMeshIndices.size() != n)
            throw std::runtime_error("reorderTLAS: the TLAS does not index every mesh once");
        std::vector<vec3> c(n);
        vec3 lo(1e30f), hi(-1e30f);
        for (size_t i = 0; i < n; ++i) {
            c[i] = world[i].center();
            for (int k = 0; k < 3; ++k) {
                lo[k] = c[i][k] < lo[k] ? c[i][k] : lo[k];
                hi[k] = c[i][k] > hi[k] ? c[i][k] : hi[k];
            }
        }
        float ext = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float e = hi[k] - lo[k];
            ext = e > ext ? e : ext;
        }
        auto spread10 = [](uint32_t v) { // 10 bits -> every third bit
            v = (v | (v << 16)) & 0x030000ffu;
            v = (v | (v << 8)) & 0x0300f00fu;
            v = (v | (v << 4)) & 0x030c30c3u;
            v = (v | (v << 2)) & 0x09249249u;
            return v;
        };
        std::vector<uint64_t> keys(n);
        for (size_t i = 0; i < n; ++i) {
            uint32_t q[3];
            for (int k = 0; k < 3; ++k) {
                float t = ext > 0.0f ? (c[i][k] - lo[k]) / ext : 0.0f;
                t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
                const int v = (int)(t * 1024.0f);
                q[k] = (uint32_t)(v > 1023 ? 1023 : v);
            }
            keys[i] = ((uint64_t)((spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2])) << 32) | (uint32_t)i;
        }
        std::sort(keys.begin(), keys.end());
        for (size_t j = 0; j < n; ++j)
            h_tlasMeshIndices[j] = (int)(uint32_t)keys[j];
    }
    // A refitted TLAS degrades as instances travel: the topology is the upload's, and the boxes of far-apart members of a leaf
    // overlap their neighbours'.  reseatTLAS() is the reference's way for the TLAS alone -- rebuilt on the host over the meshes'
    // current boxes and handed to the device with the matrices (ptrt_update_instances; synchronises) -- for a caller that wants a
    // fresh topology, say once the refitted one has cost a few per cent of frame time.
    void reseatTLAS() {
        requireUploaded("reseatTLAS");
        hostTlas = HostTlas::Current; // (rebuilt below; only the meshes' own trees have to follow the device first)
        syncHostTrees();
        for (size_t i = 0; i < meshes.size(); ++i)
            takeInstanceMove(i);
        buildTLAS();
        pointFlatAtTLAS();
        sendInstances("Failed to update the TLAS");
        instancesDirty = false;
        resetAccumulation();
    }
    // host copy of mesh `i`'s tree := what the GPU now traverses
    void syncPrimOrder(size_t i) {
        if (!getMesh(i))
            throw std::runtime_error("syncPrimOrder: no such mesh");
        readPrimOrder(i);
        meshes[i]->refitBVH();
    }

    bool hasObjectChanges() const {
        for (auto &m : meshes)
            if (m->bvhDirty)
                return true;
        return false;
    }

    // ---- quality knobs (scene.cuh:1833-1912) -----------------------------------------
    void setPerformancePreset(const std::string &p) {
        auto set = [&](bool dn, bool bl, bool mv, int depth, float scale, int rr) {
            perfSettings.enableDenoiser = dn;
            perfSettings.enableBloom = bl;
            perfSettings.enableMotionVectors = mv;
            perfSettings.maxBounceDepth = depth;
            perfSettings.resolutionScale = scale;
            perfSettings.russianRouletteStartBounce = rr;
        };
        if (p == "ultra") { set(false, true, true, 32, 1.0f, 8); perfSettings.samplesPerPixel = 128; }
        else if (p == "quality") set(true, true, true, 6, 1.0f, 2);
        else if (p == "balanced") set(true, true, true, 4, 1.0f, 1);
        else if (p == "performance") set(true, false, true, 3, 0.75f, 1);
        else if (p == "fast") set(false, false, false, 2, 0.35f, 1);
        updateScaledBuffers();
    }
    void setDenoiserEnabled(bool e) {
        if (perfSettings.enableDenoiser != e) {
            perfSettings.enableDenoiser = e;
            updateScaledBuffers(); // a no-op unless the render size changed, as in the reference
        }
    }
    void setBloomEnabled(bool e) { perfSettings.enableBloom = e; }
    void setMaxBounceDepth(int d) { perfSettings.maxBounceDepth = d < 1 ? 1 : (d > 16 ? 16 : d); }
    void setResolutionScale(float s) {
        s = fmaxf(0.25f, fminf(1.0f, s));
        if (fabsf(s - perfSettings.resolutionScale) > 0.01f) {
            perfSettings.resolutionScale = s;
            updateScaledBuffers();
        }
    }
    int getRenderWidth() const { return render_width; }
    int getRenderHeight() const { return render_height; }
    // scene.cuh:1248-1255: stored, accumulation reset -- and IGNORED by render_to_device, which takes its sample
    // count and depth from perfSettings (scene.cuh:86-87, 1044-1045).  Kept that way so a caller of the
    // reference renders the same frame here.
    void setSamplesPerPixel(int spp) { samples_per_pixel_ = spp; resetAccumulation(); }
    void setMaxDepth(int depth) { max_depth_ = depth; resetAccumulation(); }
    int getSamplesPerPixel() const { return samples_per_pixel_; } // scene.cuh:1720
    // NOT in the reference, whose perfSettings.samplesPerPixel is reachable only through the "ultra" preset
    // (scene.cuh:1839): the sample count render_to_device uses; needed to express the 4-spp configurations.
    void setPerfSamplesPerPixel(int spp) { perfSettings.samplesPerPixel = spp < 1 ? 1 : spp; }
    const PerformanceSettings &getPerformanceSettings() const { return perfSettings; }

    // ---- debug visualisation (scene.cuh:1564-1684, app_utils.cuh:304-368): out of scope -- the
    // switches and ray lists are kept so call sites compile and behave, no helper meshes are generated
    void setWireframeMode(bool e) { wireframe_mode = e; }
    bool isWireframeMode() const { return wireframe_mode; }
    void toggleWireframeMode() { wireframe_mode = !wireframe_mode; }
    void setShowFrustum(bool show) { show_frustum = show; }
    void toggleFrustum() { show_frustum = !show_frustum; }
    void setShowRays(bool show) { show_rays = show; }
    void setRayLength(float length) { ray_length = length; }
    void addDebugRay(const vec3 &origin, const vec3 &direction) { debug_rays.push_back({origin, direction, -1.0f}); }
    void addDebugRayWithLength(const vec3 &origin, const vec3 &direction, float length) {
        debug_rays.push_back({origin, direction.normalized(), length});
    }
    void clearDebugRays() { debug_rays.clear(); }
    size_t getDebugRayCount() const { return debug_rays.size(); }
    void clearVisualizationMeshes() {}
    void updateVisualizationMeshes() {
        if ((show_frustum || (show_rays && !debug_rays.empty())) && !warnedViz) {
            std::cerr << "NOTE: frustum / ray visualisation meshes are not generated by this back end\n";
            warnedViz = true;
        }
        show_frustum = false;
    }
    void generatePrimaryRayVisualization(Camera cam, int numRays = 10) {
        clearDebugRays();
        const int gridSize = (int)sqrt((double)numRays);
        for (int y = 0; y < gridSize; ++y)
            for (int x = 0; x < gridSize; ++x) {
                vec3 o, d;
                cam.get_ray((x + 0.5f) / gridSize, (y + 0.5f) / gridSize, o, d);
                addDebugRay(o, d);
            }
        std::cout << "generated primary rays" << '\n';
    }
    // scene.cuh:1211-1245: render_kernel_wireframe over the full frame (ptrt_render_wireframe), then a sync (ptrt_sync).
    // Leaves the frame counter, the accumulation, the generator states and the denoiser history alone, as the reference
    // does.  `device_pixels`: this scene's rows, bottom-up, as render_to_device writes them.
    void render_to_device_wireframe(unsigned char *device_pixels, float wireframeThickness) {
        renderWireframe(device_pixels, wireframeThickness, PTRT_OUT_DEVICE);
    }
    // the same image into HOST memory (synchronous), like render_to_host
    void render_wireframe_to_host(unsigned char *host_pixels, float wireframeThickness) {
        renderWireframe(host_pixels, wireframeThickness, PTRT_OUT_HOST);
    }
    // The baked-light view (ptrt_render_baked): the scene lit by a lightmap atlas, a probe volume, both or neither -- `view`
    // names them, with the HDR image and G-buffers to fill beside the RGB8 target (each may be null) -- at the frame index
    // render_to_device would use next, which it does not advance.  Leaves the accumulation, the generator states and the
    // denoiser history alone and does not synchronise.  `device_pixels`: this scene's rows, bottom-up; nullptr: no RGB8.
    void render_to_device_baked(unsigned char *device_pixels, const ptrt_baked_view &view) {
        renderBaked(frame_count_, device_pixels, view, PTRT_OUT_DEVICE);
    }
    // the same image into HOST memory (synchronous), like render_to_host
    void render_baked_to_host(unsigned char *host_pixels, const ptrt_baked_view &view) {
        renderBaked(frame_count_, host_pixels, view, PTRT_OUT_HOST);
    }
    // the same at a frame index of the caller's and any of ptrt_render's three targets (PTRT_OUT_DEVICE_FRAME: a band scene's
    // rows into the whole frame)
    void renderBaked(int frame, unsigned char *pixels, const ptrt_baked_view &view, int is_device) {
        if (meshes.empty()) {
            std::cerr << "Error: no meshes in scene\n";
            return;
        }
        needBackend();
        updateDeviceScene();
        check(ptrt_render_baked(ctx, frame, &view, pixels, is_device), "Baked view failed");
    }

    // ---- upload + render -------------------------------------------------------------
    void uploadToGPU() { // scene.cuh:1643-1657
        if (meshes.empty()) {
            std::cerr << "Warning: No meshes in scene\n";
            return;
        }
        if (meshes.size() != mesh_materials.size())
            throw std::runtime_error("Mesh count and material count mismatch!");
        needBackend();
        updateAccelerationStructures();
        gpu_resources_initialized = true;
        resetAccumulation();
    }

    // One frame: acceleration-structure update, path trace, tonemap into
    // `device_pixels` (W*rows*3 bytes on the device, bottom-up).  Returns without
    // synchronising, like the reference (scene.cuh:1028-1209).
    void render_to_device(unsigned char *device_pixels) { renderInternal(device_pixels, 1); }
    // same frame into HOST memory (synchronous); the reference has no such call on
    // its PT Scene -- callers there map a GL buffer instead
    void render_to_host(unsigned char *host_pixels) { renderInternal(host_pixels, 0); }
    // a band / strip scene's rows straight into the WHOLE frame (W*H*3 bytes, bottom-up, on this scene's device): what the
    // tile farm does with the parts on the presenting GPU -- no image of their own, nothing to copy (ptrt.h PTRT_OUT_DEVICE_FRAME)
    void render_to_frame(unsigned char *device_frame) { renderInternal(device_frame, PTRT_OUT_DEVICE_FRAME); }
    int deviceIndex() const { return device_; }

    // Tile farm, presenting rank: the post chain of render_to_device over a frame gathered from band contexts
    // (device pointers, top-down; include/ptrt.h ptrt_post_frame).  Same bookkeeping as a rendered frame.
    void postFrameFromDevice(const float *accum, const float *normal, const float *depth, const int *object_id,
                             unsigned char *pixels, int is_device) {
        const bool denoise = perfSettings.enableDenoiser && denoiserAllocated;
        const bool bloom = perfSettings.enableBloom && fullFrame && render_width >= 64 && render_height >= 64;
        if (fullFrame)
            check(ptrt_set_bloom(ctx, bloom ? 1 : 0), "bloom");
        if (denoiserAllocated) {
            check(ptrt_set_option(ctx, "denoiser_active", denoise ? 1 : 0), "denoiser option");
            check(ptrt_set_option(ctx, "motion_vectors", (denoise && perfSettings.enableMotionVectors) ? 1 : 0),
                  "denoiser option");
            check(ptrt_set_prev_view_proj(ctx, prev_view_proj.m), "prev view-proj");
        }
        if (cameraDirty) {
            ptrt_camera c = camera.flat();
            check(ptrt_set_camera(ctx, &c), "Failed to set camera");
            cameraDirty = false;
        }
        check(ptrt_post_frame(ctx, accum, normal, depth, object_id, pixels, is_device), "ptrt_post_frame");
        frame_count_++;
        prev_view_proj = camera.get_view_proj();
    }


    HitInfo traceSingleRay(const vec3 &o, const vec3 &d) { // scene.cuh:1367-1391
        HitInfo h;
        needBackend();
        float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
        ptrt_hit r;
        if (ptrt_trace_rays(ctx, of, df, 1, &r) != PTRT_OK) {
            std::cerr << "traceSingleRay failed: " << ptrt_last_error(ctx) << "\n";
            return h;
        }
        h.hit = r.hit != 0;
        h.t = r.t;
        h.point = vec3(r.point.x, r.point.y, r.point.z);
        h.normal = vec3(r.normal.x, r.normal.y, r.normal.z);
        h.mesh_index = r.mesh_index;
        h.front_face = r.front_face != 0;
        h.u = r.u;
        h.v = r.v;
        h.face_index = r.face_index;
        h.localPoint = vec3(r.local_point.x, r.local_point.y, r.local_point.z);
        return h;
    }

    // NOT in the reference, which answers one ray per call (traceSingleRay): batched ray queries on device memory
    // (ptrt_query_rays).  Pending object and instance changes are committed first, as a render commits them, so a query
    // sees the geometry the next frame traces.  Enqueued on the back end's stream; no synchronisation.
    // d_origins / d_dirs: n * 3 floats; d_out: n records (closest hit) or n flags (1 = blocked before d_tmax[i]).
    void queryClosestDevice(const float *d_origins, const float *d_dirs, int n, ptrt_hit *d_out) {
        needBackend();
        updateAccelerationStructures();
        check(ptrt_query_rays(ctx, PTRT_QUERY_CLOSEST, d_origins, d_dirs, nullptr, n, d_out), "Closest-hit query failed");
    }
    void queryOccludedDevice(const float *d_origins, const float *d_dirs, const float *d_tmax, int n, int32_t *d_out) {
        needBackend();
        updateAccelerationStructures();
        check(ptrt_query_rays(ctx, PTRT_QUERY_OCCLUDED, d_origins, d_dirs, d_tmax, n, d_out), "Occlusion query failed");
    }
    // Path-traced radiance for rays the caller chooses (ptrt_query_radiance): per ray tracePath with the ray's own generator
    // state (d_rng_states: n * 6 words, canonical order, advanced in place), `samples` times, the mean and the first hit of
    // sample 0 in d_out.  Everything a frame reads is committed first -- geometry, materials, lights, sky, environment map.
    // max_depth <= 0: the frame's bounce depth (perfSettings.maxBounceDepth).
    void queryRadiance(const float *d_origins, const float *d_dirs, uint32_t *d_rng_states, int n, int samples, int max_depth,
                       ptrt_radiance *d_out) {
        needBackend();
        updateDeviceScene();
        check(ptrt_query_radiance(ctx, d_origins, d_dirs, d_rng_states, n, samples,
                                  max_depth > 0 ? max_depth : perfSettings.maxBounceDepth, d_out),
              "Radiance query failed");
    }
    // Light probes (ptrt_query_probes): probe p sends n_dirs rays from d_positions[p] along the shared d_dirs, ray (p, k) with
    // generator state p * n_dirs + k (advanced in place); d_out gets one 128-byte ptrt_probe per probe -- radiance on the nine
    // spherical harmonics of bands 0-2, mean hit distance (clamped to max_distance), its square and the hit fraction, all means
    // over the directions.  Commits what queryRadiance commits.  max_depth <= 0: the frame's bounce depth.
    void queryProbes(const float *d_positions, int n_probes, const float *d_dirs, int n_dirs, uint32_t *d_rng_states, int samples,
                     int max_depth, float max_distance, ptrt_probe *d_out) {
        needBackend();
        updateDeviceScene();
        check(ptrt_query_probes(ctx, d_positions, n_probes, d_dirs, n_dirs, d_rng_states, samples,
                                max_depth > 0 ? max_depth : perfSettings.maxBounceDepth, max_distance, d_out),
              "Probe query failed");
    }
    // Lightmap texels (ptrt_query_irradiance): texel t gathers n_dirs rays from d_positions[t] + offset * d_normals[t], ray (t, k)
    // along the cosine-distributed direction the k-th point of d_samples2 (n_dirs * 2 floats in [0,1), ONE set for all texels,
    // rotated by d_phases[t] if given) maps to about the normal, with generator state t * n_dirs + k (advanced in place); d_out
    // gets one 32-byte ptrt_irradiance per texel -- mean radiance (pi times it: the irradiance), mean hit distance (clamped to
    // max_distance), its square and the hit fraction.  Commits what queryRadiance commits.  max_depth <= 0: the frame's depth.
    void queryIrradiance(const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                         const float *d_phases, float offset, uint32_t *d_rng_states, int samples, int max_depth, float max_distance,
                         ptrt_irradiance *d_out) {
        needBackend();
        updateDeviceScene();
        check(ptrt_query_irradiance(ctx, d_positions, d_normals, n_texels, d_samples2, n_dirs, d_phases, offset, d_rng_states, samples,
                                    max_depth > 0 ? max_depth : perfSettings.maxBounceDepth, max_distance, d_out),
              "Irradiance query failed");
    }
    // The rays queryIrradiance traces (ptrt_irradiance_rays): n_texels * n_dirs * 3 floats each, ray t * n_dirs + k.
    void irradianceRays(const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                        const float *d_phases, float offset, float *d_origins, float *d_dirs) {
        needBackend();
        check(ptrt_irradiance_rays(ctx, d_positions, d_normals, n_texels, d_samples2, n_dirs, d_phases, offset, d_origins, d_dirs),
              "Irradiance rays failed");
    }
    // The analytic lights' direct term at lightmap texels (ptrt_query_direct): texel t takes n_shadow light samples of each of
    // the lights light_first .. light_first + light_count - 1 (light_count < 0: all from light_first on) at d_positions[t] with
    // normal d_normals[t] -- the path tracer's own sample, its cone numbers the points of d_samples2 (n_shadow * 2 floats, rotated
    // by d_phases[t] if given) --, walks their shadow rays from d_positions[t] + offset * d_normals[t], and d_out gets one 32-byte
    // ptrt_direct per texel: the irradiance and the fractions of samples lit and shadowed.  Commits what queryRadiance commits.
    void queryDirect(const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_shadow,
                     const float *d_phases, float offset, int light_first, int light_count, ptrt_direct *d_out) {
        needBackend();
        updateDeviceScene();
        check(ptrt_query_direct(ctx, d_positions, d_normals, n_texels, d_samples2, n_shadow, d_phases, offset, light_first,
                                light_count < 0 ? (int)lights.size() - light_first : light_count, d_out),
              "Direct query failed");
    }
    // The shadow rays queryDirect walks and their weights (ptrt_direct_rays): per ray t * Q + q, Q = light_count * n_shadow, an
    // origin and a direction (3 floats each), a length and a weight (3 floats), for rays the query would not walk too.
    void directRays(const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_shadow,
                    const float *d_phases, float offset, int light_first, int light_count, float *d_origins, float *d_dirs,
                    float *d_tmax, float *d_weights) {
        needBackend();
        updateDeviceScene();
        check(ptrt_direct_rays(ctx, d_positions, d_normals, n_texels, d_samples2, n_shadow, d_phases, offset, light_first,
                               light_count < 0 ? (int)lights.size() - light_first : light_count, d_origins, d_dirs, d_tmax, d_weights),
              "Direct rays failed");
    }
    // The analytic lights' one-bounce term at lightmap texels (ptrt_query_bounce): the gather rays of queryIrradiance, and at
    // each ray's closest hit n_shadow light samples (the points of d_shadow2, rotated by d_phases[t] if given) of each of the
    // lights light_first .. light_first + light_count - 1 (light_count < 0: all from light_first on), valued by the hit's BSDF
    // as a path vertex values them and walked as shadow rays; d_out gets one 32-byte ptrt_bounce per texel -- mean radiance (pi
    // times it: the irradiance), the fractions of terms lit and shadowed, the hit fraction.  Commits what queryRadiance commits.
    void queryBounce(const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                     const float *d_phases, float offset, const float *d_shadow2, int n_shadow, int light_first, int light_count,
                     ptrt_bounce *d_out) {
        needBackend();
        updateDeviceScene();
        check(ptrt_query_bounce(ctx, d_positions, d_normals, n_texels, d_samples2, n_dirs, d_phases, offset, d_shadow2, n_shadow,
                                light_first, light_count < 0 ? (int)lights.size() - light_first : light_count, d_out),
              "Bounce query failed");
    }
    // The terms queryBounce sums (ptrt_bounce_terms) at hits the caller traced -- d_hits and d_dirs: the n_texels * n_dirs records
    // and directions of irradianceRays + a closest-hit query --: per row (t * n_dirs + k) * Q + q, Q = light_count * n_shadow, the
    // shadow ray's origin and direction (3 floats each), its length and the term's value (3 floats), walked or not.
    void bounceTerms(const ptrt_hit *d_hits, const float *d_dirs, int n_texels, int n_dirs, const float *d_shadow2, int n_shadow,
                     const float *d_phases, int light_first, int light_count, float *d_origins, float *d_L, float *d_tmax,
                     float *d_values) {
        needBackend();
        updateDeviceScene();
        check(ptrt_bounce_terms(ctx, d_hits, d_dirs, n_texels, n_dirs, d_shadow2, n_shadow, d_phases, light_first,
                                light_count < 0 ? (int)lights.size() - light_first : light_count, d_origins, d_L, d_tmax, d_values),
              "Bounce terms failed");
    }
    // A mesh's UV charts rasterised to lightmap texels (ptrt_atlas_texels): d_uv holds the (x, y) of the three corners of every
    // face of mesh `mesh` in texel units (faces * 6 floats), d_texels gets atlas_w * atlas_h 32-byte ptrt_atlas_texel -- world
    // position, geometric normal, owning face, mesh -- for the texel centres some face covers, the lowest face winning;
    // `clear` false keeps what earlier calls put there (several meshes in one atlas).  `mesh` is this scene's mesh id; the
    // record of what the device holds (Resident) says which uploaded mesh that is.  Commits what queryClosestDevice commits.
    void atlasTexels(size_t mesh, const float *d_uv, int atlas_w, int atlas_h, bool clear, ptrt_atlas_texel *d_texels) {
        needBackend();
        updateDeviceScene();
        check(ptrt_atlas_texels(ctx, residentIndex(mesh, "atlasTexels"), d_uv, atlas_w, atlas_h, clear ? 1 : 0, d_texels),
              "Atlas rasterisation failed");
    }
    // `passes` dilation passes over an atlas of float4 {r, g, b, valid} (ptrt_atlas_dilate), d_a -> d_b -> d_a ..: invalid
    // texels take the mean of their valid 8-neighbours.  Returns the buffer that holds the result.  Needs no scene.
    float *atlasDilate(float *d_a, float *d_b, int atlas_w, int atlas_h, int passes) {
        needBackend();
        check(ptrt_atlas_dilate(ctx, d_a, d_b, atlas_w, atlas_h, passes), "Atlas dilation failed");
        return (passes & 1) ? d_b : d_a;
    }
    // `passes` (1 .. 8) passes of the edge-aware a-trous filter over a baked atlas of float4 {r, g, b, valid} (ptrt_atlas_filter),
    // d_a -> d_b -> d_a .., guided by the atlas's records: pass s weighs the 25 taps of a 5 x 5 B3 kernel at step 1 << s by world
    // distance (sigma_distance * step), by distance from the centre's tangent plane (sigma_plane) and by the cosine between the
    // normals squared normal_power (0 .. 7) times.  Between scatter and atlasDilate.  Returns the buffer that holds the result.
    // Needs no scene.
    float *atlasFilter(const ptrt_atlas_texel *d_texels, float *d_a, float *d_b, int atlas_w, int atlas_h, int passes,
                       float sigma_distance, float sigma_plane, int normal_power = 2) {
        needBackend();
        check(ptrt_atlas_filter(ctx, d_texels, d_a, d_b, atlas_w, atlas_h, passes, sigma_distance, sigma_plane, normal_power),
              "Atlas filter failed");
        return (passes & 1) ? d_b : d_a;
    }
    // The baked atlas read back at ray hits (ptrt_atlas_sample): one 32-byte ptrt_lightmap_sample per ptrt_hit record of
    // queryClosestDevice -- the atlas's colour at the hit, nearest (mode PTRT_LIGHTMAP_NEAREST) or bilinear over its valid taps.
    // d_charts: the d_uv of atlasTexels for every lightmapped mesh, concatenated (n_chart_faces * 6 floats); d_chart_first: per
    // UPLOADED mesh (ptrt_hit.mesh_index counts those) the index in d_charts of its face 0, negative for a mesh without a
    // lightmap; d_image: the atlas_w * atlas_h float4 {r, g, b, valid} atlasDilate leaves.  Needs the scene for its mesh count only.
    void atlasSample(const ptrt_hit *d_hits, int n, const float *d_charts, int n_chart_faces, const int32_t *d_chart_first,
                     const float *d_image, int atlas_w, int atlas_h, int mode, ptrt_lightmap_sample *d_out) {
        needBackend();
        check(ptrt_atlas_sample(ctx, d_hits, n, d_charts, n_chart_faces, d_chart_first, d_image, atlas_w, atlas_h, mode, d_out),
              "Atlas sampling failed");
    }
    // The same for n rays traced here (ptrt_query_lightmap): what atlasSample gives for queryClosestDevice's records of these
    // rays, byte for byte, in one launch and without the records.  Commits what queryClosestDevice commits.
    void queryLightmap(const float *d_origins, const float *d_dirs, int n, const float *d_charts, int n_chart_faces,
                       const int32_t *d_chart_first, const float *d_image, int atlas_w, int atlas_h, int mode,
                       ptrt_lightmap_sample *d_out) {
        needBackend();
        updateAccelerationStructures();
        check(ptrt_query_lightmap(ctx, d_origins, d_dirs, n, d_charts, n_chart_faces, d_chart_first, d_image, atlas_w, atlas_h, mode,
                                  d_out),
              "Lightmap query failed");
    }
    // A probe volume read at surface points (ptrt_probe_sample): one 32-byte ptrt_probe_light per point -- the irradiance the
    // grid `volume` of ptrt_probe records d_probes (queryProbes' output, probe (i, j, k) in row i + nx*(j + ny*k)) gives at
    // d_positions[i] for the normal d_normals[i]: the eight probes round the point, trilinear (mode PTRT_PROBES_TRILINEAR) or
    // weighted further by facing and a Chebyshev visibility test on the probes' distance moments (PTRT_PROBES_VISIBILITY), from
    // the point moved normal_bias along its normal.  Needs no scene.
    void probeSample(const float *d_positions, const float *d_normals, int n, const ptrt_probe_volume &volume, const ptrt_probe *d_probes,
                     int mode, float normal_bias, ptrt_probe_light *d_out) {
        needBackend();
        check(ptrt_probe_sample(ctx, d_positions, d_normals, n, &volume, d_probes, mode, normal_bias, d_out), "Probe sampling failed");
    }
    // The same for n rays traced here (ptrt_query_probe_light): what probeSample gives for the point and normal columns of
    // queryClosestDevice's records of these rays, byte for byte, with the hit's face and mesh, in one launch and without the
    // records.  Commits what queryClosestDevice commits.
    void queryProbeLight(const float *d_origins, const float *d_dirs, int n, const ptrt_probe_volume &volume, const ptrt_probe *d_probes,
                         int mode, float normal_bias, ptrt_probe_light *d_out) {
        needBackend();
        updateAccelerationStructures();
        check(ptrt_query_probe_light(ctx, d_origins, d_dirs, n, &volume, d_probes, mode, normal_bias, d_out), "Probe light query failed");
    }
    // The primary rays render_to_device would give sample `sample` of frame `frame` (ptrt_camera_rays; pinhole cameras only):
    // tile rows * width * 3 floats each, in the order of the colour buffer.
    void cameraRays(int frame, int sample, float *d_origins, float *d_dirs) {
        needBackend();
        updateDeviceScene();
        check(ptrt_camera_rays(ctx, frame, sample, d_origins, d_dirs), "Camera rays failed");
    }
    // n fresh generator states for subsequences first .. first + n - 1 of `seed` (ptrt_init_rng_states), n * 6 words.
    void initRngStates(unsigned long long seed, unsigned long long first, int n, uint32_t *d_states) {
        needBackend();
        check(ptrt_init_rng_states(ctx, seed, first, n, d_states), "Generator states failed");
    }

    void saveAsPPM(const std::string &filename, unsigned char *pixels) const { // ASCII P3, scene.cuh:1694-1708
        std::ofstream ofs(filename, std::ios::binary);
        if (!ofs)
            throw std::runtime_error("Cannot open file: " + filename);
        ofs << "P3\n" << width << ' ' << height << "\n255\n";
        for (size_t i = 0, n = (size_t)width * height * 3; i < n; i += 3)
            ofs << int(pixels[i]) << ' ' << int(pixels[i + 1]) << ' ' << int(pixels[i + 2]) << '\n';
    }

    int getWidth() const { return width; }
    int getHeight() const { return height; }
    int getTileRows() const { return tileRows; } // rows this context renders (== height unless it is a band)
    int getTileY0() const { return tileY0; }
    int getDevice() const { return device_; }
    size_t getPixelBufferSize() const { return (size_t)width * height * 3; }
    int getFrameCount() const { return frame_count_; }
    // DEVICE pointers, as in the reference (scene.cuh:1722-1725)
    vec3 *getNoisyColorBuffer() { return (vec3 *)ptrt_device_buffer(ctx, PTRT_BUF_ACCUM); }
    vec3 *getNormalBuffer() { return (vec3 *)ptrt_device_buffer(ctx, PTRT_BUF_NORMAL); }
    float *getDepthBuffer() { return (float *)ptrt_device_buffer(ctx, PTRT_BUF_DEPTH); }
    int *getObjectIdBuffer() { return (int *)ptrt_device_buffer(ctx, PTRT_BUF_OBJECT_ID); }
    float *getMotionVectorBuffer() { return (float *)ptrt_device_buffer(ctx, PTRT_BUF_MOTION); } // float2 per pixel
    vec3 *getDenoisedBuffer() { return (vec3 *)ptrt_device_buffer(ctx, PTRT_BUF_DENOISED); }
    mat4 getPrevViewProjMatrix() const { return prev_view_proj; }
    mat4 getViewProjMatrix() const { return camera.get_view_proj(); }

    // ---- access for tests, tools and the tile farm -----------------------------------
    ptrt_ctx *backend() { return ctx; }
    void setFrameCount(int f) { frame_count_ = f; }
    // Flattened view of the current scene (pointers stay valid until the next
    // mutation of the scene).  Brings BLAS/TLAS up to date first.
    const ptrt_scene_desc &flatten() {
        prepareHostStructures();
        return flat;
    }

  private:
    int width, height, tileRows = 0, tileY0 = 0, device_ = 0;
    int samples_per_pixel_ = 16, max_depth_ = 8; // scene.cuh:86-87: stored, ignored by render_to_device
    int frame_count_ = 0;
    struct DebugRay {
        vec3 origin, direction;
        float length; // < 0: the scene's ray_length
    };
    std::vector<DebugRay> debug_rays;
    bool wireframe_mode = false, show_frustum = false, show_rays = false, warnedViz = false;
    float ray_length = 5.0f;
    int bvhLeafTarget_ = 12, bvhLeafTol_ = 5; // scene.cuh:90-91
    std::vector<std::unique_ptr<Mesh>> meshes;
    std::vector<Material> mesh_materials;
    std::vector<Light> lights;
    Camera camera;
    bool use_sky = true;
    vec3 sky_color_top{0.6f, 0.7f, 1.0f}, sky_color_bottom{1.0f, 1.0f, 1.0f}; // scene.cuh:164-166
    PerformanceSettings perfSettings;
    bool gpu_resources_initialized = false;

    ptrt_ctx *ctx = nullptr;
    bool geometryDirty = true, materialsDirty = true, lightsDirty = true, cameraDirty = true, skyDirty = true;
    bool instancesDirty = false; // only instance transforms (and with them the TLAS) changed since the last upload
    bool warnedPost = false, denoiserAllocated = false;
    std::vector<float> envMap;                // RGBA floats of the HDRI sky (empty: gradient)
    int env_width = 0, env_height = 0;
    bool envDirty = false;
    bool fullFrame = false;                   // band (tile) contexts have no post chain
    int render_width = 0, render_height = 0;  // scene.cuh:203-204
    mat4 prev_view_proj; // proj*view of the previous frame (scene.cuh:113)

    // scene.cuh:1913-2000: the size the path tracer renders at follows perfSettings.resolutionScale
    // (>= 64, and here also <= the frame); when it changes, the low-resolution buffers and the
    // denoiser are re-created (the denoiser only if enabled) and accumulation restarts.
    void updateScaledBuffers() {
        int nw = static_cast<int>(width * perfSettings.resolutionScale);
        int nh = static_cast<int>(height * perfSettings.resolutionScale);
        nw = nw < 64 ? 64 : nw;
        nh = nh < 64 ? 64 : nh;
        nw = nw > width ? width : nw;
        nh = nh > height ? height : nh;
        if (nw == render_width && nh == render_height)
            return;
        if (ctx && !fullFrame)
            return; // a band context always renders its rows of the full-size frame
        render_width = nw;
        render_height = nh;
        if (ctx) {
            check(ptrt_set_render_size(ctx, nw, nh), "Failed to resize the render buffers");
            denoiserAllocated = false; // freed by the resize
            if (perfSettings.enableDenoiser) {
                check(ptrt_denoiser_enable(ctx, nullptr), "Failed to create denoiser");
                denoiserAllocated = true;
            }
        }
        resetAccumulation();
    }

    // flattened arrays handed to the back end
    std::vector<ptrt_mesh_desc> flatMeshes;
    std::vector<mat4> lastWorld;
    std::vector<DeviceBVHNode> h_tlasNodes;
    std::vector<int> h_tlasMeshIndices;
    std::vector<ptrt_light> flatLights;
    struct MatSoA {
        std::vector<ptrt_vec3> albedo, specular, emission, subsurfaceColor, sheenTint;
        std::vector<float> metallic, roughness, ior, transmission, transmissionRoughness, clearcoat,
            clearcoatRoughness, subsurfaceRadius, anisotropy, sheen, iridescence, iridescenceThickness;
    } soa;
    ptrt_scene_desc flat{};
    // What the device holds of one mesh since the last ptrt_upload_geometry, and whether the host copy of its tree still equals
    // the device's: BoxesStale -- the device refitted it (Mesh::refitBVH brings the host copy up); OrderStale -- the device
    // rebuilt it (the prim order is read back first).  A mark only grows until syncHostTrees() consumes it: an order read-back
    // stays pending across later refits.
    enum class HostTree : unsigned char { Current, BoxesStale, OrderStale };
    struct Resident {
        size_t verts = 0, faceCount = 0;
        std::vector<Tri> faces; // kept under a non-default policy only (HostRebuild pays nothing for the copy)
        bool soup = false;      // `faces` is the unshared-vertex pattern {3k, 3k+1, 3k+2} (sameFaces)
        HostTree hostTree = HostTree::Current;
        void mark(HostTree t) { hostTree = t > hostTree ? t : hostTree; }
    };
    std::vector<Resident> resident;
    // the uploaded index of this scene's mesh `mesh`: meshes are uploaded in the scene's order, one Resident record each
    int residentIndex(size_t mesh, const char *who) const {
        if (mesh >= resident.size() || mesh >= meshes.size() || resident[mesh].faceCount != meshes[mesh]->faces.size())
            throw std::runtime_error(std::string(who) + ": mesh " + std::to_string(mesh) + " is not on the device (" +
                                     std::to_string(resident.size()) + " uploaded)");
        return (int)mesh;
    }
    // the same for the TLAS: the device refitted it (ptrt_refit_tlas) over root boxes the host has not followed yet, or
    // re-ordered it as well (ptrt_reorder_tlas: the index array is read back with the boxes)
    enum class HostTlas : unsigned char { Current, BoxesStale, OrderStale };
    HostTlas hostTlas = HostTlas::Current;
    void markHostTlas(HostTlas t) { hostTlas = t > hostTlas ? t : hostTlas; }
    DynamicGeometryPolicy dynPolicy = DynamicGeometryPolicy::HostRebuild;
    size_t gpuDynamicCommits = 0, geometryUploads = 0;
    double commitMicros = 0.0, compareMicros = 0.0;
    struct Timer { // adds its lifetime, in microseconds, to `acc`
        double &acc;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Timer() { acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
    };

    void needBackend() const {
        if (!ctx)
            throw std::runtime_error("host-only Scene (device < 0) has no GPU back end");
    }
    void check(int rc, const char *what) {
        if (rc != PTRT_OK)
            throw std::runtime_error(std::string(what) + ": " + ptrt_last_error(ctx));
    }
    Mesh *push(std::unique_ptr<Mesh> m, const Material &mat) {
        meshes.push_back(std::move(m));
        mesh_materials.push_back(mat);
        geometryDirty = materialsDirty = true;
        resetAccumulation();
        return meshes.back().get();
    }
    void addLight(const Light &l) {
        lights.push_back(l);
        lightsDirty = true;
        resetAccumulation();
    }

    // ---- small pieces every route below shares ----
    // (one form for every caller: after an upload without geometryDirty the descriptors are sized and the TLAS exists, so the two
    // extra conditions refitInstanceChanges / reorderTLAS used to name alone refuse nothing the others accepted)
    void requireUploaded(const char *who) const {
        needBackend();
        if (!gpu_resources_initialized || geometryDirty || flatMeshes.size() != meshes.size() || h_tlasNodes.empty())
            throw std::runtime_error(std::string(who) + ": call uploadToGPU() first (the geometry and the TLAS topology must already be on the GPU)");
    }
    // the matrices and the has_transform rule of a descriptor (ptrt_mesh_desc) or of an instance record (ptrt_instance_xform)
    template <class Desc> static void writeInstance(Desc &d, const Transform3D &t) {
        std::memcpy(d.world, t.worldMatrix.m, sizeof d.world);
        std::memcpy(d.inverse, t.inverseMatrix.m, sizeof d.inverse);
        std::memcpy(d.normal, t.normalMatrix.m, sizeof d.normal);
        d.has_transform = (t.position.length() > 0.001f || t.rotation.length() > 0.001f || fabsf(t.scale.x - 1.0f) > 0.001f)
                              ? 1
                              : 0; // scene.cuh:718-721 (only scale.x is inspected)
    }
    // mesh i's instance transform is not the one its descriptor was last written from
    bool instanceMoved(size_t i) const {
        const Transform3D &t = meshes[i]->transform;
        return t.dirty || std::memcmp(&lastWorld[i], &t.worldMatrix, sizeof(mat4)) != 0;
    }
    // ... then matrices, descriptor and lastWorld are brought up to date, as prepareHostStructures does; false if nothing changed
    bool takeInstanceMove(size_t i) {
        if (!instanceMoved(i))
            return false;
        Transform3D &t = meshes[i]->transform;
        t.updateMatrices();
        lastWorld[i] = t.worldMatrix;
        writeInstance(flatMeshes[i], t);
        return true;
    }
    // mesh i's world box as every TLAS takes it: its root node's box through Transform3D::transformAABB
    AABB meshWorldBox(size_t i) const {
        const Mesh *m = meshes[i].get();
        if (m->bvhNodes.empty())
            throw std::runtime_error("Mesh BVH not built before TLAS");
        const DeviceBVHNode &root = m->bvhNodes[0];
        return m->transform.transformAABB(AABB{vec3(root.bmin.x, root.bmin.y, root.bmin.z), vec3(root.bmax.x, root.bmax.y, root.bmax.z)});
    }
    void pointFlatAtTLAS() {
        flat.tlas_nodes = h_tlasNodes.data();
        flat.tlas_node_count = (int)h_tlasNodes.size();
        flat.tlas_mesh_indices = h_tlasMeshIndices.data();
        flat.tlas_index_count = (int)h_tlasMeshIndices.size();
    }
    void sendInstances(const char *what) { // every descriptor's matrices and the host's TLAS (synchronises)
        check(ptrt_update_instances(ctx, flat.meshes, flat.mesh_count, flat.tlas_nodes, flat.tlas_node_count, flat.tlas_mesh_indices,
                                    flat.tlas_index_count),
              what);
    }
    void readPrimOrder(size_t i) { // (synchronises)
        Mesh *m = meshes[i].get();
        check(ptrt_read_prim_order(ctx, (int)i, m->bvhPrimIndices.data(), (int)m->bvhPrimIndices.size()), "Failed to read the prim order");
    }
    // the host TLAS over the topology it has, optionally re-ordered first as ptrt_reorder_tlas re-orders the device's
    void refitHostTLAS(bool reorder) {
        const std::vector<AABB> world = meshWorldBoxes();
        if (reorder)
            mortonOrderTLAS(world);
        refitTLASNode(0, world, 0);
    }
    void moveInstancesOnHost(const char *who, bool reorder) {
        if (geometryDirty && ctx)
            throw std::runtime_error(std::string(who) + ": geometry is dirty");
        if (flatMeshes.size() != meshes.size() || h_tlasNodes.empty())
            prepareHostStructures();
        for (size_t i = 0; i < meshes.size(); ++i)
            takeInstanceMove(i);
        refitHostTLAS(reorder);
        resetAccumulation();
    }
    AABB refitTLASNode(int n, const std::vector<AABB> &world, int depth) {
        if (n < 0 || n >= (int)h_tlasNodes.size() || depth > 64)
            throw std::runtime_error("refitTLAS: malformed TLAS");
        DeviceBVHNode &N = h_tlasNodes[n];
        AABB b = AABB::make_invalid();
        if (N.count > 0) {
            for (int k = 0; k < N.count; ++k)
                b.expand(world[(size_t)h_tlasMeshIndices[(size_t)N.start + k]]);
        } else {
            if (N.left >= 0)
                b.expand(refitTLASNode(N.left, world, depth + 1));
            if (N.right >= 0)
                b.expand(refitTLASNode(N.right, world, depth + 1));
        }
        N.bmin = {b.bmin.x, b.bmin.y, b.bmin.z};
        N.bmax = {b.bmax.x, b.bmax.y, b.bmax.z};
        return b;
    }
    // TLAS over the meshes' world AABBs, same builder and leaf limit as the BLAS
    // (scene.cuh:458-594)
    void buildTLAS() {
        std::vector<ptrt_detail::BuildRef> refs(meshes.size());
        for (size_t i = 0; i < meshes.size(); ++i) {
            meshes[i]->transform.updateMatrices();
            const AABB world = meshWorldBox(i);
            refs[i].id = (int)i;
            refs[i].b = world;
            refs[i].c = world.center();
        }
        h_tlasNodes.clear();
        h_tlasMeshIndices.clear();
        ptrt_detail::build_bvh_range(refs, 0, (int)refs.size(), bvhLeafTarget_ + bvhLeafTol_, h_tlasNodes,
                                     h_tlasMeshIndices);
    }

    // host half of updateAccelerationStructures (scene.cuh:596-743): rebuild dirty
    // BLAS, refresh descriptors, detect moved instances, rebuild the TLAS
    // `forRead`: somebody is about to read the host trees (flatten()).  A commit that stays on the GPU does not: the host copy
    // of a tree the GPU refitted / rebuilt is brought up to date only when it is read or uploaded again -- before a full upload,
    // for a TLAS with inner nodes (rebuilt on the host over the new boxes), when an instance moved (its world box comes from
    // the tree's root) -- not on every commit (a CPU refit of the whole tree, and after a GPU rebuild a read-back that waits
    // for the stream).
    void prepareHostStructures(bool forRead = true) {
        if (meshes.empty())
            return;
        // (a TLAS the DEVICE refitted needs no host trees until something reads or moves them)
        bool need_trees = forRead || geometryDirty || flatMeshes.size() != meshes.size() || (h_tlasNodes.size() != 1 && hostTlas == HostTlas::Current);
        for (size_t i = 0; i < meshes.size() && !need_trees; ++i) {
            const Mesh *m = meshes[i].get();
            need_trees = m->vertsDirty || m->bvhDirty || m->bvhNodes.empty() || instanceMoved(i);
        }
        const bool synced = need_trees && syncHostTrees(); // (trees the GPU refitted / rebuilt since the host last looked)
        // (refitted trees move the box of a single-leaf TLAS; one with inner nodes was refitted on the device and read back)
        bool tlas_dirty = h_tlasNodes.empty() || (synced && h_tlasNodes.size() == 1);
        if (flatMeshes.size() != meshes.size()) {
            flatMeshes.assign(meshes.size(), ptrt_mesh_desc{});
            lastWorld.assign(meshes.size(), mat4());
            tlas_dirty = true;
            geometryDirty = materialsDirty = true;
        }
        for (size_t i = 0; i < meshes.size(); ++i) {
            Mesh *m = meshes[i].get();
            if (m->vertsDirty) {
                geometryDirty = true;
                m->vertsDirty = false;
            }
            if (m->bvhDirty || m->bvhNodes.empty()) {
                m->setBVHLeafParams(bvhLeafTarget_, bvhLeafTol_);
                m->buildBVH();
                tlas_dirty = true;
                geometryDirty = true;
            }
            if (instanceMoved(i)) { // an instance moved: new matrices + TLAS, the triangles stay (ptrt_update_instances)
                tlas_dirty = true;
                instancesDirty = true;
            }
            m->transform.updateMatrices();
            lastWorld[i] = m->transform.worldMatrix;
            ptrt_mesh_desc &d = flatMeshes[i];
            d.verts = reinterpret_cast<const ptrt_vec3 *>(m->vertices.data());
            d.vert_count = (int)m->vertices.size();
            d.faces = m->faces.data();
            d.face_count = (int)m->faces.size();
            d.nodes = m->bvhNodes.data();
            d.node_count = (int)m->bvhNodes.size();
            d.prim_indices = m->bvhPrimIndices.data();
            d.prim_count = (int)m->bvhPrimIndices.size();
            writeInstance(d, m->transform);
        }
        if (tlas_dirty)
            buildTLAS();

        // materials: AoS -> SoA (scene.cuh:286-431)
        const size_t n = mesh_materials.size();
        auto c = [](const vec3 &a) { return ptrt_vec3{a.x, a.y, a.z}; };
        soa.albedo.resize(n); soa.specular.resize(n); soa.emission.resize(n); soa.subsurfaceColor.resize(n);
        soa.sheenTint.resize(n); soa.metallic.resize(n); soa.roughness.resize(n); soa.ior.resize(n);
        soa.transmission.resize(n); soa.transmissionRoughness.resize(n); soa.clearcoat.resize(n);
        soa.clearcoatRoughness.resize(n); soa.subsurfaceRadius.resize(n); soa.anisotropy.resize(n);
        soa.sheen.resize(n); soa.iridescence.resize(n); soa.iridescenceThickness.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const Material &m = mesh_materials[i];
            soa.albedo[i] = c(m.albedo); soa.specular[i] = c(m.specular); soa.emission[i] = c(m.emission);
            soa.subsurfaceColor[i] = c(m.subsurfaceColor); soa.sheenTint[i] = c(m.sheenTint);
            soa.metallic[i] = m.metallic; soa.roughness[i] = m.roughness; soa.ior[i] = m.ior;
            soa.transmission[i] = m.transmission; soa.transmissionRoughness[i] = m.transmissionRoughness;
            soa.clearcoat[i] = m.clearcoat; soa.clearcoatRoughness[i] = m.clearcoatRoughness;
            soa.subsurfaceRadius[i] = m.subsurfaceRadius; soa.anisotropy[i] = m.anisotropy; soa.sheen[i] = m.sheen;
            soa.iridescence[i] = m.iridescence; soa.iridescenceThickness[i] = m.iridescenceThickness;
        }
        flatLights.resize(lights.size());
        for (size_t i = 0; i < lights.size(); ++i) {
            const Light &l = lights[i];
            flatLights[i] = ptrt_light{(int32_t)l.type, c(l.position), c(l.direction), c(l.color), l.intensity,
                                       l.range, l.innerCone, l.outerCone, l.radius};
        }
        flat.meshes = flatMeshes.data();
        flat.mesh_count = (int)flatMeshes.size();
        pointFlatAtTLAS();
        flat.materials = ptrt_materials{soa.albedo.data(), soa.specular.data(), soa.metallic.data(),
                                        soa.roughness.data(), soa.emission.data(), soa.ior.data(),
                                        soa.transmission.data(), soa.transmissionRoughness.data(),
                                        soa.clearcoat.data(), soa.clearcoatRoughness.data(),
                                        soa.subsurfaceColor.data(), soa.subsurfaceRadius.data(),
                                        soa.anisotropy.data(), soa.sheen.data(), soa.sheenTint.data(),
                                        soa.iridescence.data(), soa.iridescenceThickness.data(), (int32_t)n};
        flat.lights = flatLights.data();
        flat.light_count = (int)flatLights.size();
        flat.camera = camera.flat();
        flat.sky_top = c(sky_color_top);
        flat.sky_bottom = c(sky_color_bottom);
        flat.use_sky = use_sky ? 1 : 0;
        flat.env_rgba = envMap.empty() ? nullptr : envMap.data();
        flat.env_width = env_width;
        flat.env_height = env_height;
    }

    // ---- the one route of a device-side geometry edit ----
    // An edit: new positions for mesh `mesh` from host or device memory -- all `count` vertices (ptrt_update_vertices), or
    // `count` triangles of a soup with room for more (ptrt_update_triangles).
    struct VertexEdit {
        size_t mesh;
        const float *data;
        int count;
        bool onDevice, triangles;
    };
    enum class Trees { Refit, Rebuild }; // one ptrt_refit over every mesh, or ptrt_build_bvh per edited mesh
    // The host copy of an edited tree: brought up at once (a rebuild's prim order read back, boxes refitted); marked in its
    // Resident record for syncHostTrees() and the mesh's dirty flags taken -- always, or only behind a TLAS with inner nodes
    // (else the mesh stays dirty for the next commit's host rebuild); or left behind: the caller keeps no host copy.
    enum class HostTrees { FollowNow, Marked, MarkedBehindInnerNodes, LeftBehind };
    // The TLAS over the moved root boxes: rebuilt on the host over its CURRENT trees and sent if it has inner nodes (syncTLAS;
    // a single leaf got its box from ptrt_refit / ptrt_build_bvh); only if it has inner nodes, the marked trees synced first,
    // a single leaf's host copy following lazily; refitted on the device if it has inner nodes, the host's marked stale; moved
    // instances' matrices sent and refitted there; or left alone.
    enum class Tlas { RebuiltOnHost, RebuiltBehindInnerNodes, RefittedOnDevice, RefittedOnDeviceWithMoves, Untouched };

    VertexEdit hostVertices(size_t i) const { return {i, &meshes[i]->vertices[0].x, (int)meshes[i]->vertices.size(), false, false}; }
    VertexEdit vertexEdit(const char *who, size_t mesh, const float *data, bool onDevice, int triangles = -1) const {
        needBackend();
        if (!getMesh(mesh))
            throw std::runtime_error(std::string(who) + ": no such mesh");
        return {mesh, data, triangles < 0 ? (int)meshes[mesh]->vertices.size() : triangles, onDevice, triangles >= 0};
    }
    // every mesh whose vertices the caller rewrote in place, as an edit from its host copy; the flag is taken
    std::vector<VertexEdit> takeVertsDirty() {
        std::vector<VertexEdit> edits;
        for (size_t i = 0; i < meshes.size(); ++i)
            if (meshes[i]->vertsDirty) {
                meshes[i]->vertsDirty = false;
                edits.push_back(hostVertices(i));
            }
        return edits;
    }
    void editOnDevice(const std::vector<VertexEdit> &edits, Trees trees, HostTrees host, Tlas tlas) {
        for (const VertexEdit &e : edits) {
            if (e.triangles)
                check(ptrt_update_triangles(ctx, (int)e.mesh, e.data, e.count, e.onDevice ? 1 : 0), "Failed to update triangles");
            else
                check(ptrt_update_vertices(ctx, (int)e.mesh, e.data, e.count, e.onDevice ? 1 : 0), "Failed to update vertices");
            if (trees == Trees::Rebuild)
                check(ptrt_build_bvh(ctx, (int)e.mesh), "Failed to build BVH");
            hostTreeFollows(e, trees, host);
        }
        if (trees == Trees::Refit)
            check(ptrt_refit(ctx), "Failed to refit");
        tlasFollows(tlas);
    }
    void hostTreeFollows(const VertexEdit &e, Trees trees, HostTrees how) {
        Mesh *m = meshes[e.mesh].get();
        if (how == HostTrees::FollowNow) {
            for (size_t v = 0, real = (size_t)e.count * 3; e.triangles && v < m->vertices.size(); ++v) {
                const size_t s = v < real ? v : (real ? real - 1 : 0); // (the padded vertices the device now holds)
                m->vertices[v] = real ? vec3(e.data[s * 3], e.data[s * 3 + 1], e.data[s * 3 + 2]) : vec3(0.0f);
            }
            if (trees == Trees::Rebuild)
                readPrimOrder(e.mesh);
            m->refitBVH();
        } else if (how == HostTrees::Marked || (how == HostTrees::MarkedBehindInnerNodes && h_tlasNodes.size() > 1)) {
            resident[e.mesh].mark(trees == Trees::Rebuild ? HostTree::OrderStale : HostTree::BoxesStale);
            m->bvhDirty = m->vertsDirty = false;
            flatMeshes[e.mesh].verts = reinterpret_cast<const ptrt_vec3 *>(m->vertices.data()); // (the caller may have re-allocated them)
            flatMeshes[e.mesh].faces = m->faces.data();
        }
    }
    void tlasFollows(Tlas how) {
        const bool inner = h_tlasNodes.size() > 1; // (the one place the TLAS's shape decides; hostTreeFollows has the trees')
        if (how == Tlas::RebuiltBehindInnerNodes && inner)
            syncHostTrees();
        if (how == Tlas::RebuiltOnHost || (how == Tlas::RebuiltBehindInnerNodes && inner)) {
            syncTLAS();
        } else if (how == Tlas::RefittedOnDeviceWithMoves) {
            refitMovedInstances();
        } else if (how == Tlas::RefittedOnDevice && inner) {
            check(ptrt_refit_tlas(ctx), "Failed to refit the TLAS");
            markHostTlas(HostTlas::BoxesStale);
        }
    }

    // The dynamic-geometry policy (setDynamicGeometryPolicy): meshes whose vertices changed while their topology is what
    // the device holds keep their uploaded tree.  Returns false when the commit has to take the reference's route.
    bool commitOnGpu() {
        if (dynPolicy == DynamicGeometryPolicy::HostRebuild || !gpu_resources_initialized || geometryDirty ||
            resident.size() != meshes.size() || flatMeshes.size() != meshes.size())
            return false;
        std::vector<VertexEdit> edits;
        for (size_t i = 0; i < meshes.size(); ++i) {
            const Mesh *m = meshes[i].get();
            if (!m->bvhDirty && !m->vertsDirty)
                continue;
            if (m->bvhNodes.empty() || m->vertices.size() != resident[i].verts || m->faces.size() != resident[i].faces.size())
                return false;
            if (!sameFaces(*m, resident[i]))
                return false;
            edits.push_back(hostVertices(i));
        }
        const bool all = dynPolicy == DynamicGeometryPolicy::GpuRefitAll;
        bool instances = false;
        for (size_t i = 0; all && i < meshes.size() && !instances; ++i)
            instances = instanceMoved(i);
        if (edits.empty() && !instances)
            return false;
        // under GpuRefitAll the TLAS is refitted on the device and rebuilt nowhere; else a real TLAS is rebuilt on the host over
        // the new boxes, as the reference's commit does, and a single leaf needs nothing
        const Tlas tlas = !all ? Tlas::RebuiltBehindInnerNodes : instances ? Tlas::RefittedOnDeviceWithMoves : Tlas::RefittedOnDevice;
        if (edits.empty())
            tlasFollows(tlas); // (instances alone moved: no vertices, no refit)
        else
            editOnDevice(edits, dynPolicy == DynamicGeometryPolicy::GpuRebuild ? Trees::Rebuild : Trees::Refit, HostTrees::Marked, tlas);
        ++gpuDynamicCommits;
        return true;
    }
    // Is the face list of mesh m what the device holds?  A `Triangles` mesh as updatePTScene rewrites it (PTRTtransfer.cuh:2249-2270)
    // is an unshared-vertex soup: face k = {3k, 3k+1, 3k+2}.  If the uploaded list was that soup (noted at upload), the new
    // list is checked against the PATTERN -- one pass over 12 bytes per face, no second array to stream -- else word by word
    // against the copy kept from the upload.
    bool sameFaces(const Mesh &m, const Resident &r) {
        Timer timer{compareMicros};
        if (r.soup) {
            const Tri *f = m.faces.data();
            const int n = (int)m.faces.size();
            int bad = 0;
            for (int k = 0; k < n; ++k) // (branch-free: the compiler vectorises it)
                bad |= (f[k].v0 ^ (3 * k)) | (f[k].v1 ^ (3 * k + 1)) | (f[k].v2 ^ (3 * k + 2));
            return bad == 0;
        }
        return std::memcmp(m.faces.data(), r.faces.data(), r.faces.size() * sizeof(Tri)) == 0;
    }
    // what the device holds of mesh i := the host arrays as they stand -- after an upload, or for a mesh nobody has touched
    // since when a policy is chosen later; the host-tree mark is not this function's
    void recordResident(size_t i) {
        const Mesh &m = *meshes[i];
        Resident &r = resident[i];
        r.verts = m.vertices.size();
        r.faceCount = m.faces.size();
        r.faces.clear();
        r.soup = false;
        if (dynPolicy == DynamicGeometryPolicy::HostRebuild)
            return;
        r.faces = m.faces;
        r.soup = r.faces.size() * 3 == r.verts;
        for (size_t k = 0; r.soup && k < r.faces.size(); ++k)
            r.soup = r.faces[k].v0 == (int)(3 * k) && r.faces[k].v1 == (int)(3 * k + 1) && r.faces[k].v2 == (int)(3 * k + 2);
    }
    // host copies of the trees the GPU refitted (boxes) or rebuilt (prim order, then boxes); true if any changed.  A marked mesh
    // whose arrays are no longer the size the device holds was resized by the caller since: its tree cannot describe them (a
    // refit would index past their ends), so the mark is dropped and the mesh left dirty for the host rebuild of this commit.
    bool syncHostTrees() {
        bool any = false;
        for (size_t i = 0; i < resident.size() && i < meshes.size(); ++i) {
            Resident &r = resident[i];
            const HostTree was = r.hostTree;
            if (was == HostTree::Current)
                continue;
            r.hostTree = HostTree::Current;
            Mesh *m = meshes[i].get();
            if (m->vertices.size() != r.verts || m->faces.size() != r.faceCount) {
                m->bvhDirty = true;
                continue;
            }
            if (was == HostTree::OrderStale && ctx)
                readPrimOrder(i);
            const bool bd = m->bvhDirty; // (a caller's later edit stays pending)
            m->refitBVH();
            m->bvhDirty = bd;
            any = true;
        }
        if (hostTlas != HostTlas::Current && ctx && !h_tlasNodes.empty()) { // the TLAS as the device refitted it (ptrt_read_tlas synchronises)
            if (hostTlas == HostTlas::OrderStale)
                check(ptrt_read_tlas_order(ctx, h_tlasMeshIndices.data(), (int)h_tlasMeshIndices.size()), "Failed to read the TLAS order");
            check(ptrt_read_tlas(ctx, h_tlasNodes.data(), (int)h_tlasNodes.size()), "Failed to read the TLAS");
            hostTlas = HostTlas::Current;
        }
        return any;
    }

    void updateAccelerationStructures() {
        if (meshes.empty())
            return;
        Timer timer{commitMicros};
        if (!ctx) { // host-only scene: the host half of a commit (trees, TLAS, material arrays); there is nothing to upload to
            prepareHostStructures();
            return;
        }
        commitOnGpu();
        prepareHostStructures(false);
        if (geometryDirty) {
            check(ptrt_upload_geometry(ctx, flat.meshes, flat.mesh_count, flat.tlas_nodes, flat.tlas_node_count,
                                       flat.tlas_mesh_indices, flat.tlas_index_count),
                  "Failed to upload geometry");
            geometryDirty = instancesDirty = false;
            hostTlas = HostTlas::Current;
            ++geometryUploads;
            resident.assign(meshes.size(), Resident{}); // what the device now holds
            for (size_t i = 0; i < meshes.size(); ++i)
                recordResident(i);
        } else if (instancesDirty) {
            sendInstances("Failed to update instances");
            instancesDirty = false;
            hostTlas = HostTlas::Current;
        }
        if (materialsDirty) {
            check(ptrt_upload_materials(ctx, &flat.materials), "Failed to upload materials");
            materialsDirty = false;
        }
        if (lightsDirty) {
            check(ptrt_upload_lights(ctx, flat.lights, flat.light_count), "Failed to upload lights");
            lightsDirty = false;
        }
        gpu_resources_initialized = true;
    }

    // the acceleration structures, then the camera, sky and environment map the back end caches: what a frame reads
    void updateDeviceScene() {
        updateAccelerationStructures();
        if (cameraDirty) {
            ptrt_camera c = camera.flat();
            check(ptrt_set_camera(ctx, &c), "Failed to set camera");
            cameraDirty = false;
        }
        if (skyDirty) {
            ptrt_vec3 t{sky_color_top.x, sky_color_top.y, sky_color_top.z},
                b{sky_color_bottom.x, sky_color_bottom.y, sky_color_bottom.z};
            check(ptrt_set_sky(ctx, &t, &b, use_sky ? 1 : 0), "Failed to set sky");
            skyDirty = false;
        }
        if (envDirty) {
            check(ptrt_set_env_map(ctx, envMap.empty() ? nullptr : envMap.data(), env_width, env_height),
                  "Failed to upload the environment map");
            envDirty = false;
        }
    }

    void renderWireframe(unsigned char *pixels, float thickness, int is_device) {
        if (meshes.empty()) {
            std::cerr << "Error: no meshes in scene\n";
            return;
        }
        needBackend();
        updateDeviceScene();
        check(ptrt_render_wireframe(ctx, thickness, pixels, is_device), "Wireframe kernel failed");
        check(ptrt_sync(ctx), "Wireframe kernel failed"); // cudaDeviceSynchronize (scene.cuh:1244)
    }

    void renderInternal(unsigned char *pixels, int is_device) {
        // validateGPUResources: message on cerr and return without rendering (scene.cuh:216-251,1029-1031)
        if (meshes.empty()) {
            std::cerr << "ERROR: No meshes in scene!\n";
            return;
        }
        if (!gpu_resources_initialized) {
            std::cerr << "ERROR: Mesh descriptors not allocated!\n";
            return;
        }
        const bool denoise = perfSettings.enableDenoiser && denoiserAllocated;
        // bloom (scene.cuh:1137-1183) needs the whole frame and six non-empty mip levels
        const bool bloom = perfSettings.enableBloom && fullFrame && render_width >= 64 && render_height >= 64;
        if (((perfSettings.enableBloom && !bloom) || (!fullFrame && (perfSettings.enableDenoiser ||
                                                                     perfSettings.resolutionScale != 1.0f))) &&
            !warnedPost) {
            std::cerr << "NOTE: " << (fullFrame ? "bloom needs a frame of at least 64x64 pixels and is skipped\n"
                                                : "a band (tile) context renders its rows only: denoiser, bloom and "
                                                  "resolution scaling are skipped (apply them on the presenting rank)\n");
            warnedPost = true;
        }
        if (fullFrame)
            check(ptrt_set_bloom(ctx, bloom ? 1 : 0), "bloom");
        if (denoiserAllocated) { // scene.cuh:1103-1127: motion vectors + Denoiser::denoise after the trace
            check(ptrt_set_option(ctx, "denoiser_active", denoise ? 1 : 0), "denoiser option");
            check(ptrt_set_option(ctx, "motion_vectors", (denoise && perfSettings.enableMotionVectors) ? 1 : 0),
                  "denoiser option");
            check(ptrt_set_prev_view_proj(ctx, prev_view_proj.m), "prev view-proj");
        }
        updateDeviceScene();
        int rc = ptrt_render(ctx, frame_count_, perfSettings.samplesPerPixel, perfSettings.maxBounceDepth, pixels,
                             is_device);
        if (rc != PTRT_OK) // launch errors are logged, not thrown (scene.cuh:1036-1042)
            std::cerr << "HIP kernel launch failed at path_trace_kernel: " << ptrt_last_error(ctx) << "\n";
        frame_count_++;
        prev_view_proj = camera.get_view_proj(); // scene.cuh:1208
    }
};
