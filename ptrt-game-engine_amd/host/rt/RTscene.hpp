// rt/RTscene.hpp -- host mirror of the ray tracer's Scene API (src/raytracer/RTscene.cuh:21-80, 765-1236, 1297-1590).
//
// Everything lives in namespace ptrt_rt: the path tracer's mirror (host/ptrt/) has global Scene / Mesh / Material /
// Light / Camera classes in the same library.  A Scene made with device = HOST_ONLY builds and inspects scenes without
// a GPU; a device scene sends its meshes, trees, descriptors and lights through the ptrt_rt_* entries of
// include/ptrt.h and renders with rt_render_kernel (csrc/rt_render.hip.h).
#pragma once
#include "../../../include/ptrt.h"
#include "RTcamera.hpp"
#include "RTmesh.hpp"

#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace ptrt_rt {

constexpr int HOST_ONLY = -1;

struct Material { // RTscene.cuh:21-61
    vec3 albedo = vec3(0.8f), specular = vec3(0.04f);
    float metallic = 0.0f, roughness = 0.5f;
    vec3 emission = vec3(0.0f);
    float ior = 1.5f, transmission = 0.0f, transmissionRoughness = 0.0f, clearcoat = 0.0f, clearcoatRoughness = 0.03f;
    vec3 subsurfaceColor = vec3(1.0f);
    float subsurfaceRadius = 0.0f, anisotropy = 0.0f, sheen = 0.0f;
    vec3 sheenTint = vec3(0.5f);
    float iridescence = 0.0f, iridescenceThickness = 550.0f;

    Material() = default;
    Material(const vec3 &alb, float rough = 0.5f, float met = 0.0f) : albedo(alb), metallic(met), roughness(rough) {
        specular = lerp(vec3(0.04f), albedo, metallic);
    }
};

enum LightType { LIGHT_POINT = 0, LIGHT_DIRECTIONAL = 1, LIGHT_SPOT = 2 };

struct Light { // RTscene.cuh:64-80
    LightType type = LIGHT_POINT;
    vec3 position = vec3(0, 10, 0), direction = vec3(0, -1, 0), color = vec3(1.0f);
    float intensity = 1.0f, range = 100.0f, innerCone = 0.5f, outerCone = 0.7f;
};

struct mat3 { // common/matrix.cuh: row-major, identity by default
    float m[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    mat3 operator*(const mat3 &o) const {
        mat3 r;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                r.m[i][j] = 0;
                for (int k = 0; k < 3; k++)
                    r.m[i][j] += m[i][k] * o.m[k][j];
            }
        return r;
    }
    mat3 transpose() const {
        mat3 r;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                r.m[i][j] = m[j][i];
        return r;
    }
};
inline mat3 rows3(float a, float b, float c, float d, float e, float f, float g, float h, float i) {
    mat3 r;
    const float v[9] = {a, b, c, d, e, f, g, h, i};
    for (int k = 0; k < 9; ++k)
        r.m[k / 3][k % 3] = v[k];
    return r;
}
inline mat3 rotation_x(float a) { return rows3(1, 0, 0, 0, std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a)); }
inline mat3 rotation_y(float a) { return rows3(std::cos(a), 0, std::sin(a), 0, 1, 0, -std::sin(a), 0, std::cos(a)); }
inline mat3 rotation_z(float a) { return rows3(std::cos(a), -std::sin(a), 0, std::sin(a), std::cos(a), 0, 0, 0, 1); }

inline ptrt_vec3 pv(const vec3 &v) { return ptrt_vec3{v.x, v.y, v.z}; }

class Scene {
    int width, height, device;
    int bvhLeafTarget_ = 4, bvhLeafTol_ = 2;
    std::vector<std::unique_ptr<Mesh>> meshes;
    std::vector<Material> mesh_materials;
    std::vector<Light> lights;
    Camera camera;
    vec3 ambient_light = vec3(0.1f);
    bool use_sky = true;
    vec3 sky_color_top = vec3(0.6f, 0.7f, 1.0f), sky_color_bottom = vec3(1.0f, 1.0f, 1.0f);
    ptrt_rt_ctx *ctx = nullptr;
    bool uploaded = false;

  public:
    // what the last upload / render sent (Scene::snapshot of the binding)
    std::vector<ptrt_rt_mesh> sentMeshes;
    std::vector<ptrt_rt_light> sentLights;
    ptrt_rt_view sentView{};
    bool viewSent = false;

    Scene(int w, int h, int dev = 0) : width(w), height(h), device(dev), camera(static_cast<float>(w) / h, 2.0f, 1.0f) {
        if (device != HOST_ONLY) {
            const int rc = ptrt_rt_create(w, h, device, &ctx);
            if (rc != PTRT_OK)
                throw std::runtime_error(std::string("Scene: ") + ptrt_rt_last_error(nullptr));
        }
    }
    ~Scene() { ptrt_rt_destroy(ctx); }
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    Mesh *getMesh(size_t i) { return i < meshes.size() ? meshes[i].get() : nullptr; }
    size_t getMeshCount() const { return meshes.size(); }
    size_t getLightCount() const { return lights.size(); }
    const Material &getMeshMaterial(size_t i) const { return mesh_materials.at(i); }
    const Light &getLight(size_t i) const { return lights.at(i); }
    vec3 getAmbientLight() const { return ambient_light; }
    bool getUseSky() const { return use_sky; }
    vec3 getSkyTop() const { return sky_color_top; }
    vec3 getSkyBottom() const { return sky_color_bottom; }
    bool isHostOnly() const { return ctx == nullptr; }

    void setBVHLeafTarget(int target, int tol = 2) {
        bvhLeafTarget_ = target < 1 ? 1 : target;
        bvhLeafTol_ = tol < 0 ? 0 : tol;
        for (auto &m : meshes)
            m->bvhDirty = true;
    }
    void setMeshMaterial(size_t i, const Material &mat) {
        if (i < mesh_materials.size())
            mesh_materials[i] = mat;
    }
    void setCamera(const vec3 &lookfrom, const vec3 &lookat, const vec3 &vup, float vfov, float aperture = 0.0f,
                   float focus_dist = 1.0f) {
        camera = Camera(lookfrom, lookat, vup, vfov, static_cast<float>(width) / height, aperture, focus_dist);
    }
    void setCameraSimple(float viewport_height = 2.0f, float focal_length = 1.0f) {
        camera = Camera(static_cast<float>(width) / height, viewport_height, focal_length);
    }
    vec3 cameraOrigin() const { return camera.get_origin(); }
    vec3 cameraForward() const {
        return (camera.get_lower_left_corner() + camera.get_horizontal() * 0.5f + camera.get_vertical() * 0.5f - camera.get_origin())
            .normalized();
    }
    void moveCamera(const vec3 &pos) { camera.set_position(pos); }
    void lookCameraAt(const vec3 &target, const vec3 &vup = vec3(0, 1, 0)) { camera.look_at(target, vup); }

    Mesh *addMesh(const std::string &obj_path, const Material &mat = Material()) {
        meshes.push_back(std::make_unique<Mesh>(obj_path));
        mesh_materials.push_back(mat);
        return meshes.back().get();
    }
    // one mesh of independent triangles (v0, v1, v2 per 9 floats)
    Mesh *addTriangles(const std::vector<vec3> &corners, const Material &mat = Material()) {
        auto m = std::make_unique<Mesh>();
        m->vertices.clear();
        m->faces.clear();
        for (size_t i = 0; i + 2 < corners.size(); i += 3) {
            const int base = (int)m->vertices.size();
            m->vertices.push_back(corners[i]);
            m->vertices.push_back(corners[i + 1]);
            m->vertices.push_back(corners[i + 2]);
            m->faces.push_back(Tri{base, base + 1, base + 2});
        }
        meshes.push_back(std::move(m));
        mesh_materials.push_back(mat);
        return meshes.back().get();
    }
    Mesh *addPlaneXZ(float y, float half, const Material &mat = Material(vec3(0.8f))) {
        const vec3 A(-half, y, -half), B(half, y, -half), C(half, y, half), D(-half, y, half);
        return addTriangles({A, C, B, A, D, C}, mat);
    }
    Mesh *addSphere(int segments = 32, const Material &mat = Material(vec3(1.0f, 0.0f, 0.0f))) {
        auto m = std::make_unique<Mesh>();
        m->vertices.clear();
        m->faces.clear();
        const float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f, radius = 0.5f;
        for (int r = 0; r <= segments; ++r) {
            const float phi = kPi * float(r) / float(segments);
            const float y = std::cos(phi) * radius, ring = std::sin(phi) * radius;
            for (int s = 0; s <= segments; ++s) {
                const float theta = kTwoPi * float(s) / float(segments);
                m->vertices.push_back(vec3(ring * std::cos(theta), y, ring * std::sin(theta)));
            }
        }
        for (int r = 0; r < segments; ++r)
            for (int s = 0; s < segments; ++s) {
                const int curr = r * (segments + 1) + s, next = curr + segments + 1;
                m->faces.push_back({curr, next, curr + 1});
                m->faces.push_back({curr + 1, next, next + 1});
            }
        meshes.push_back(std::move(m));
        mesh_materials.push_back(mat);
        return meshes.back().get();
    }
    void addCheckerboardPlaneXZ(float y, int tiles, float tileSize, const Material &whiteMat, const Material &blackMat) {
        std::vector<vec3> white, black;
        const float start = -tiles * tileSize;
        for (int iz = 0; iz < 2 * tiles; ++iz)
            for (int ix = 0; ix < 2 * tiles; ++ix) {
                const float x0 = start + ix * tileSize, x1 = x0 + tileSize, z0 = start + iz * tileSize, z1 = z0 + tileSize;
                const vec3 A(x0, y, z0), B(x1, y, z0), C(x1, y, z1), D(x0, y, z1);
                auto &b = ((ix + iz) & 1) == 0 ? white : black;
                for (const vec3 &p : {A, C, B, A, D, C})
                    b.push_back(p);
            }
        if (!white.empty())
            addTriangles(white, whiteMat);
        if (!black.empty())
            addTriangles(black, blackMat);
    }
    Mesh *addCube(const Material &mat = Material(vec3(1.0f, 0.0f, 0.0f))) {
        meshes.push_back(std::make_unique<Mesh>());
        mesh_materials.push_back(mat);
        return meshes.back().get();
    }

    void addPointLight(const vec3 &position, const vec3 &color, float intensity = 1.0f, float range = 100.0f) {
        Light l;
        l.type = LIGHT_POINT;
        l.position = position;
        l.color = color;
        l.intensity = intensity;
        l.range = range;
        lights.push_back(l);
    }
    void addDirectionalLight(const vec3 &direction, const vec3 &color, float intensity = 1.0f) {
        Light l;
        l.type = LIGHT_DIRECTIONAL;
        l.direction = direction.normalized();
        l.color = color;
        l.intensity = intensity;
        lights.push_back(l);
    }
    void addSpotLight(const vec3 &position, const vec3 &direction, const vec3 &color, float intensity = 1.0f,
                      float innerCone = 0.5f, float outerCone = 0.7f, float range = 100.0f) {
        Light l;
        l.type = LIGHT_SPOT;
        l.position = position;
        l.direction = direction.normalized();
        l.color = color;
        l.intensity = intensity;
        l.innerCone = std::cos(innerCone);
        l.outerCone = std::cos(outerCone);
        l.range = range;
        lights.push_back(l);
    }
    void setAmbientLight(const vec3 &a) { ambient_light = a; }
    void setSkyGradient(const vec3 &top, const vec3 &bottom) {
        sky_color_top = top;
        sky_color_bottom = bottom;
        use_sky = true;
    }
    void disableSky() { use_sky = false; }

    // Scene::uploadToGPU (RTscene.cuh:1031-1100)
    void uploadToGPU() {
        if (meshes.empty()) {
            std::fprintf(stderr, "Warning: no meshes in scene\n");
            return;
        }
        sync_descriptors();
        uploaded = true;
    }
    // Scene::render (RTscene.cuh:1102-1132): the LAST upload's meshes and lights, the current camera, ambient and sky
    void render(unsigned char *output_pixels) {
        if (!uploaded || meshes.empty()) {
            std::fprintf(stderr, "Error: Scene not uploaded to GPU\n");
            return;
        }
        launch(output_pixels, PTRT_OUT_HOST);
    }
    // Scene::render_to_device (RTscene.cuh:1134-1210): descriptors and lights rebuilt on every call
    void render_to_device(unsigned char *device_pixels) {
        if (meshes.empty()) {
            std::fprintf(stderr, "Error: no meshes in scene\n");
            return;
        }
        sync_descriptors();
        uploaded = true;
        launch(device_pixels, PTRT_OUT_DEVICE);
    }

    void saveAsPPM(const std::string &filename, const unsigned char *pixels) const {
        std::ofstream ofs(filename, std::ios::binary);
        if (!ofs)
            throw std::runtime_error("Cannot open file: " + filename);
        ofs << "P3\n" << width << ' ' << height << "\n255\n";
        size_t idx = 0;
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x, idx += 3)
                ofs << int(pixels[idx]) << ' ' << int(pixels[idx + 1]) << ' ' << int(pixels[idx + 2]) << '\n';
    }

    int getWidth() const { return width; }
    int getHeight() const { return height; }
    size_t getPixelBufferSize() const { return static_cast<size_t>(width) * height * 3; }
    Camera &getCamera() { return camera; }

  private:
    static void check(int rc, const char *what) {
        if (rc != PTRT_OK)
            throw std::runtime_error(std::string(what) + ": " + ptrt_rt_last_error(nullptr));
    }
    static bool same_geometry(const Mesh &m) {
        return m.sentVertices.size() == m.vertices.size() && m.sentFaces.size() == m.faces.size() &&
               (m.vertices.empty() || !std::memcmp(m.sentVertices.data(), m.vertices.data(), m.vertices.size() * sizeof(vec3))) &&
               (m.faces.empty() || !std::memcmp(m.sentFaces.data(), m.faces.data(), m.faces.size() * sizeof(Tri)));
    }
    // The per-mesh part of uploadToGPU / render_to_device: Mesh::upload, a rebuild + uploadBVH when the tree is dirty
    // (or was never sent), the descriptor.  Geometry the device already holds is not sent again; a direct edit of
    // `vertices` without bvhDirty is sent and walked with the OLD tree, as in the reference.
    void sync_descriptors() {
        sentMeshes.assign(meshes.size(), ptrt_rt_mesh{});
        for (size_t i = 0; i < meshes.size(); ++i) {
            Mesh &m = *meshes[i];
            const bool first = i >= sentCount;
            if (first || !same_geometry(m)) {
                if (ctx)
                    check(ptrt_rt_upload_mesh(ctx, (int)i, reinterpret_cast<const ptrt_vec3 *>(m.vertices.data()), (int)m.vertices.size(),
                                              reinterpret_cast<const ptrt_tri *>(m.faces.data()), (int)m.faces.size()),
                          "uploadToGPU");
                m.sentVertices = m.vertices;
                m.sentFaces = m.faces;
            }
            if (m.bvhDirty || !m.sentTree || m.sentNodes.empty()) {
                m.setBVHLeafParams(bvhLeafTarget_, bvhLeafTol_);
                m.buildBVH();
                if (ctx)
                    check(ptrt_rt_upload_bvh(ctx, (int)i, reinterpret_cast<const ptrt_bvh_node *>(m.bvhNodes.data()), (int)m.bvhNodes.size(),
                                             m.bvhPrimIndices.data(), (int)m.bvhPrimIndices.size()),
                          "uploadToGPU");
                m.sentNodes = m.bvhNodes;
                m.sentPrims = m.bvhPrimIndices;
                m.sentTree = true;
            }
            ptrt_rt_mesh &d = sentMeshes[i];
            const Material &mt = mesh_materials[i];
            d.material = ptrt_rt_material{pv(mt.albedo), pv(mt.specular), mt.metallic, mt.roughness, pv(mt.emission), mt.ior,
                                          mt.transmission, mt.transmissionRoughness, mt.clearcoat, mt.clearcoatRoughness,
                                          pv(mt.subsurfaceColor), mt.subsurfaceRadius, mt.anisotropy, mt.sheen, pv(mt.sheenTint),
                                          mt.iridescence, mt.iridescenceThickness};
            const mat3 R = rotation_y(m.rotationEuler.y) * rotation_x(m.rotationEuler.x) * rotation_z(m.rotationEuler.z);
            const mat3 Ri = R.transpose();
            d.translation = pv(m.position);
            std::memcpy(d.rotation, R.m, sizeof d.rotation);
            std::memcpy(d.inv_rotation, Ri.m, sizeof d.inv_rotation);
        }
        sentCount = std::max(sentCount, meshes.size());
        sentLights.clear();
        for (const Light &l : lights)
            sentLights.push_back(ptrt_rt_light{(int32_t)l.type, pv(l.position), pv(l.direction), pv(l.color), l.intensity, l.range,
                                               l.innerCone, l.outerCone});
        if (ctx)
            check(ptrt_rt_set_scene(ctx, sentMeshes.data(), (int)sentMeshes.size(), sentLights.data(), (int)sentLights.size()),
                  "uploadToGPU");
    }
    void launch(void *out, int is_device) {
        sentView = ptrt_rt_view{pv(camera.get_origin()), pv(camera.get_corner_minus_origin()), pv(camera.get_horizontal()),
                                pv(camera.get_vertical()), pv(ambient_light), pv(sky_color_top), pv(sky_color_bottom),
                                use_sky ? 1 : 0};
        viewSent = true;
        if (!ctx)
            throw std::runtime_error("render: a HOST_ONLY scene cannot render");
        check(ptrt_rt_render(ctx, &sentView, out, is_device), "render");
    }
    size_t sentCount = 0;
};

// The presets of the reference's namespace Materials (RTscene.cuh:1297-1590).  Each is Material(albedo, roughness,
// metallic) -- specular = lerp(0.04, albedo, metallic) -- followed by the field values the preset sets, in its order.
namespace Materials {
namespace detail {
template <class F> Material tuned(const vec3 &albedo, float rough, float metal, F &&set) {
    Material m(albedo, rough, metal);
    set(m);
    return m;
}
inline void dielectric(Material &m, float transmission, float ior) {
    m.transmission = transmission;
    m.ior = ior;
}
inline void coat(Material &m, float amount, float rough) {
    m.clearcoat = amount;
    m.clearcoatRoughness = rough;
}
inline void sss(Material &m, const vec3 &colour, float radius) {
    m.subsurfaceColor = colour;
    m.subsurfaceRadius = radius;
}
inline void film(Material &m, float amount, float thickness) {
    m.iridescence = amount;
    m.iridescenceThickness = thickness;
}
// the three polished / honed stones: roughness, clearcoat and clearcoat roughness per finish, IOR 1.49, subsurface
inline Material stone(const vec3 &albedo, bool polished, const float (&pol)[3], const float (&honed)[3], const vec3 &sub, float radius) {
    const float *k = polished ? pol : honed;
    return tuned(albedo, k[0], 0.0f, [&](Material &m) {
        m.ior = 1.49f;
        coat(m, k[1], k[2]);
        sss(m, sub, radius);
    });
}
} // namespace detail
using detail::tuned;

// metals: the specular colour is the albedo's (Gold's a little warmer)
inline Material Gold() { return tuned(vec3(1.0f, 0.766f, 0.336f), 0.1f, 1.0f, [](Material &m) { m.specular = vec3(1.0f, 0.782f, 0.344f); }); }
inline Material Silver() { return tuned(vec3(0.972f, 0.960f, 0.915f), 0.1f, 1.0f, [](Material &m) { m.specular = m.albedo; }); }
inline Material Copper() { return tuned(vec3(0.955f, 0.637f, 0.538f), 0.1f, 1.0f, [](Material &m) { m.specular = m.albedo; }); }
inline Material Bronze() { return tuned(vec3(0.8f, 0.5f, 0.2f), 0.25f, 0.9f, [](Material &m) { m.specular = vec3(0.7f, 0.4f, 0.15f); }); }
inline Material Aluminum() { return tuned(vec3(0.913f, 0.921f, 0.925f), 0.2f, 1.0f, [](Material &m) { m.specular = m.albedo; }); }
inline Material BrushedAluminum() {
    return tuned(vec3(0.913f, 0.921f, 0.925f), 0.35f, 1.0f, [](Material &m) { m.specular = m.albedo; m.anisotropy = 0.8f; });
}
inline Material Iron() { return tuned(vec3(0.560f, 0.570f, 0.580f), 0.4f, 1.0f, [](Material &m) { m.specular = m.albedo; }); }
inline Material Chrome() { return tuned(vec3(0.549f, 0.556f, 0.554f), 0.02f, 1.0f, [](Material &m) { m.specular = m.albedo; }); }

// transmissive
inline Material Glass() { return tuned(vec3(1.0f), 0.0f, 0.0f, [](Material &m) { detail::dielectric(m, 1.0f, 1.5f); m.specular = vec3(0.04f); }); }
inline Material FrostedGlass() {
    return tuned(vec3(1.0f), 0.0f, 0.0f, [](Material &m) {
        detail::dielectric(m, 1.0f, 1.5f);
        m.transmissionRoughness = 0.3f;
        m.roughness = 0.3f;
        m.specular = vec3(0.04f);
    });
}
inline Material Diamond() { return tuned(vec3(1.0f), 0.0f, 0.0f, [](Material &m) { detail::dielectric(m, 1.0f, 2.42f); m.specular = vec3(0.17f); }); }
inline Material Water() {
    return tuned(vec3(0.8f, 0.95f, 1.0f), 0.01f, 0.0f, [](Material &m) { detail::dielectric(m, 0.9f, 1.33f); m.specular = vec3(0.02f); });
}
inline Material SoapBubble() {
    return tuned(vec3(1.0f), 0.0f, 0.0f, [](Material &m) {
        detail::dielectric(m, 0.95f, 1.33f);
        detail::film(m, 1.0f, 380.0f);
        m.specular = vec3(0.04f);
    });
}
inline Material Ice() {
    return tuned(vec3(0.9f, 0.95f, 1.0f), 0.1f, 0.0f, [](Material &m) {
        detail::dielectric(m, 0.7f, 1.31f);
        detail::sss(m, vec3(0.8f, 0.9f, 1.0f), 0.3f);
    });
}

// dielectrics with a plain specular level
inline Material PlasticRed() { return tuned(vec3(0.8f, 0.1f, 0.1f), 0.2f, 0.0f, [](Material &m) { m.specular = vec3(0.04f); }); }
inline Material PlasticBlue() { return tuned(vec3(0.1f, 0.2f, 0.8f), 0.2f, 0.0f, [](Material &m) { m.specular = vec3(0.04f); }); }
inline Material PlasticGreen() { return tuned(vec3(0.1f, 0.7f, 0.2f), 0.2f, 0.0f, [](Material &m) { m.specular = vec3(0.04f); }); }
inline Material RubberBlack() { return tuned(vec3(0.05f), 0.8f, 0.0f, [](Material &m) { m.specular = vec3(0.03f); }); }
inline Material Cotton(const vec3 &c) { return tuned(c, 0.9f, 0.0f, [](Material &m) { m.specular = vec3(0.02f); }); }
inline Material Concrete() { return tuned(vec3(0.5f, 0.5f, 0.5f), 0.9f, 0.0f, [](Material &m) { m.specular = vec3(0.02f); }); }
inline Material WoodOak() { return tuned(vec3(0.6f, 0.4f, 0.2f), 0.5f, 0.0f, [](Material &m) { m.specular = vec3(0.04f); }); }
inline Material WoodCherry() { return tuned(vec3(0.5f, 0.2f, 0.1f), 0.4f, 0.0f, [](Material &m) { detail::coat(m, 0.3f, 0.1f); }); }
inline Material WoodWalnut() { return tuned(vec3(0.3f, 0.2f, 0.15f), 0.45f, 0.0f, [](Material &m) { m.specular = vec3(0.04f); }); }

// coated paints
inline Material CarPaint(const vec3 &base) {
    return tuned(base, 0.2f, 0.3f, [](Material &m) { detail::coat(m, 1.0f, 0.03f); m.specular = vec3(0.05f); });
}
inline Material PearlescentPaint(const vec3 &base) {
    Material m = CarPaint(base);
    detail::film(m, 0.8f, 400.0f);
    return m;
}

// subsurface
inline Material Skin() {
    return tuned(vec3(0.95f, 0.75f, 0.67f), 0.4f, 0.0f, [](Material &m) { detail::sss(m, vec3(1.0f, 0.4f, 0.3f), 0.5f); m.specular = vec3(0.028f); });
}
inline Material Wax() {
    return tuned(vec3(0.95f, 0.93f, 0.88f), 0.3f, 0.0f, [](Material &m) { detail::sss(m, vec3(1.0f, 0.9f, 0.7f), 0.8f); m.specular = vec3(0.03f); });
}
inline Material Jade() {
    return tuned(vec3(0.2f, 0.6f, 0.4f), 0.1f, 0.0f, [](Material &m) { detail::sss(m, vec3(0.3f, 0.8f, 0.5f), 0.3f); m.specular = vec3(0.05f); });
}
inline Material MarbleCarrara(bool polished = true) {
    return detail::stone(vec3(0.93f, 0.94f, 0.96f), polished, {0.15f, 0.70f, 0.05f}, {0.35f, 0.15f, 0.20f}, vec3(0.98f, 0.98f, 0.96f), 1.0f);
}
inline Material MarbleNero(bool polished = true) {
    return detail::stone(vec3(0.04f, 0.045f, 0.05f), polished, {0.12f, 0.85f, 0.04f}, {0.28f, 0.20f, 0.18f}, vec3(0.15f, 0.15f, 0.16f), 0.6f);
}
inline Material MarbleVerde(bool polished = true) {
    return detail::stone(vec3(0.10f, 0.18f, 0.14f), polished, {0.14f, 0.75f, 0.05f}, {0.30f, 0.18f, 0.19f}, vec3(0.12f, 0.20f, 0.16f), 0.8f);
}

// cloth
inline Material Velvet(const vec3 &c) {
    return tuned(c, 0.8f, 0.0f, [&](Material &m) { m.sheen = 1.0f; m.sheenTint = c * 1.2f; m.specular = vec3(0.02f); });
}
inline Material Silk(const vec3 &c) {
    return tuned(c, 0.2f, 0.0f, [](Material &m) { m.sheen = 0.6f; m.sheenTint = vec3(1.0f); m.anisotropy = 0.5f; m.specular = vec3(0.04f); });
}

// thin film over a dark metal; emitters
inline Material OilSlick() { return tuned(vec3(0.01f), 0.0f, 0.95f, [](Material &m) { detail::film(m, 1.0f, 450.0f); }); }
inline Material EmissiveLamp(const vec3 &c, float intensity = 5.0f) {
    return tuned(vec3(1.0f), 0.0f, 0.0f, [&](Material &m) { m.emission = c * intensity; });
}
inline Material NeonLight(const vec3 &c) { return tuned(c * 0.1f, 0.0f, 0.0f, [&](Material &m) { m.emission = c * 10.0f; }); }
} // namespace Materials

// The reference's namespace Scenes (RTscene.cuh:1594-1633): three unit cubes (red, blue, gold) over the default
// camera, a point, a directional and a spot light, a blue-grey ambient and sky.
namespace Scenes {
inline std::unique_ptr<Scene> createLitTestScene(int width = 800, int height = 600, int device = 0) {
    auto scene = std::make_unique<Scene>(width, height, device);
    const struct {
        Material mat;
        vec3 at;
    } cubes[3] = {{Materials::tuned(vec3(0.8f, 0.2f, 0.2f), 0.2f, 0.0f, [](Material &m) { m.specular = vec3(0.5f); }), vec3(-2, 0, -5)},
                  {Materials::tuned(vec3(0.2f, 0.2f, 0.8f), 0.3f, 0.0f, [](Material &m) { m.specular = vec3(0.3f); }), vec3(2, 0, -5)},
                  {Materials::tuned(vec3(0.9f, 0.7f, 0.3f), 0.15f, 1.0f, [](Material &m) { m.specular = vec3(0.8f, 0.6f, 0.2f); }),
                   vec3(0, 2, -5)}};
    for (const auto &c : cubes) {
        Mesh *m = scene->addCube(c.mat);
        m->moveTo(c.at);
        m->scale(0.8f);
    }
    scene->addPointLight(vec3(5, 5, 0), vec3(1.0f, 0.9f, 0.8f), 2.0f, 50.0f);
    scene->addDirectionalLight(vec3(-0.3f, -0.8f, -0.5f), vec3(0.9f, 0.9f, 1.0f), 0.5f);
    scene->addSpotLight(vec3(0, 4, -2), vec3(0, -1, -0.3f), vec3(1.0f, 0.8f, 0.6f), 3.0f, 0.3f, 0.5f, 20.0f);
    scene->setAmbientLight(vec3(0.05f, 0.05f, 0.08f));
    scene->setSkyGradient(vec3(0.5f, 0.6f, 0.9f), vec3(0.9f, 0.9f, 0.95f));
    return scene;
}
} // namespace Scenes

} // namespace ptrt_rt
