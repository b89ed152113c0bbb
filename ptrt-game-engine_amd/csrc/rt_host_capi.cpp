// rt_host_capi.cpp -- flat C entry points (hrt_*) of the ray tracer's host mirror (host/rt/RTscene.hpp), one per
// mirror method, for the Python binding ptrt_amd.rt.  A translation unit of its own: the path tracer's mirror
// (ptrt_host_capi.cpp) has global classes of the same names.  Every entry returns 0 / a value >= 0 on success and -1
// after an exception or a bad handle, with the message in hrt_last_error().
#include "../host/rt/RTscene.hpp"

#include <cstring>
#include <initializer_list>
#include <mutex>
#include <set>
#include <string>

using namespace ptrt_rt;

namespace {
thread_local std::string g_err;
std::mutex g_mu;
std::set<Scene *> g_scenes;

bool live(Scene *s) {
    std::lock_guard<std::mutex> lock(g_mu);
    return s && g_scenes.count(s);
}
Material to_mat(const ptrt_rt_material *m) {
    Material r;
    if (!m)
        return r;
    auto v = [](ptrt_vec3 p) { return vec3(p.x, p.y, p.z); };
    r.albedo = v(m->albedo);
    r.specular = v(m->specular);
    r.metallic = m->metallic;
    r.roughness = m->roughness;
    r.emission = v(m->emission);
    r.ior = m->ior;
    r.transmission = m->transmission;
    r.transmissionRoughness = m->transmission_roughness;
    r.clearcoat = m->clearcoat;
    r.clearcoatRoughness = m->clearcoat_roughness;
    r.subsurfaceColor = v(m->subsurface_color);
    r.subsurfaceRadius = m->subsurface_radius;
    r.anisotropy = m->anisotropy;
    r.sheen = m->sheen;
    r.sheenTint = v(m->sheen_tint);
    r.iridescence = m->iridescence;
    r.iridescenceThickness = m->iridescence_thickness;
    return r;
}
void from_mat(const Material &m, ptrt_rt_material *o) {
    *o = ptrt_rt_material{pv(m.albedo), pv(m.specular), m.metallic, m.roughness, pv(m.emission), m.ior, m.transmission,
                          m.transmissionRoughness, m.clearcoat, m.clearcoatRoughness, pv(m.subsurfaceColor), m.subsurfaceRadius,
                          m.anisotropy, m.sheen, pv(m.sheenTint), m.iridescence, m.iridescenceThickness};
}
vec3 v3(const float *p) { return vec3(p[0], p[1], p[2]); }

template <class F> int guard(Scene *s, const char *what, F &&f, std::initializer_list<const void *> need = {}) {
    for (const void *p : need)
        if (!p) {
            g_err = std::string(what) + ": NULL argument";
            return -1;
        }
    if (!live(s)) {
        g_err = std::string(what) + ": bad scene handle";
        return -1;
    }
    try {
        return f(*s);
    } catch (const std::exception &e) {
        g_err = std::string(what) + ": " + e.what();
        return -1;
    }
}
template <class F> int guard_mesh(Scene *s, int i, const char *what, F &&f, std::initializer_list<const void *> need = {}) {
    return guard(
        s, what,
        [&](Scene &S) {
            Mesh *m = S.getMesh((size_t)i);
            if (i < 0 || !m)
                throw std::runtime_error("no mesh " + std::to_string(i));
            return f(S, *m);
        },
        need);
}
} // namespace

extern "C" {

const char *hrt_last_error() { return g_err.c_str(); }

Scene *hrt_create(int w, int h, int device) {
    try {
        if (w <= 0 || h <= 0)
            throw std::runtime_error("bad frame size");
        Scene *s = new Scene(w, h, device);
        std::lock_guard<std::mutex> lock(g_mu);
        g_scenes.insert(s);
        return s;
    } catch (const std::exception &e) {
        g_err = std::string("hrt_create: ") + e.what();
        return nullptr;
    }
}
void hrt_destroy(Scene *s) {
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!s || !g_scenes.count(s))
            return;
        g_scenes.erase(s);
    }
    delete s;
}

// Material(albedo, roughness, metallic) and the presets of namespace Materials
int hrt_material_make(const float *albedo, float rough, float metal, ptrt_rt_material *out) {
    if (!albedo || !out)
        return -1;
    from_mat(Material(v3(albedo), rough, metal), out);
    return 0;
}
int hrt_material_default(ptrt_rt_material *out) {
    if (!out)
        return -1;
    from_mat(Material(), out);
    return 0;
}
// a preset of namespace Materials by name; `colour` (3 floats) is the argument of CarPaint, PearlescentPaint, Velvet,
// Silk, Cotton, EmissiveLamp and NeonLight, `arg` EmissiveLamp's intensity or the marbles' `polished` (non-zero)
int hrt_material_preset(const char *name, const float *colour, float arg, ptrt_rt_material *out) {
    if (!name || !out) {
        g_err = "hrt_material_preset: NULL argument";
        return -1;
    }
    const std::string n = name;
    const vec3 c = colour ? v3(colour) : vec3(1.0f);
    const bool pol = arg != 0.0f;
    using namespace Materials;
    const std::pair<const char *, Material (*)()> plain[] = {
        {"Gold", Gold}, {"Silver", Silver}, {"Copper", Copper}, {"Bronze", Bronze}, {"Aluminum", Aluminum},
        {"BrushedAluminum", BrushedAluminum}, {"Iron", Iron}, {"Chrome", Chrome}, {"Glass", Glass}, {"FrostedGlass", FrostedGlass},
        {"Diamond", Diamond}, {"Water", Water}, {"SoapBubble", SoapBubble}, {"Ice", Ice}, {"PlasticRed", PlasticRed},
        {"PlasticBlue", PlasticBlue}, {"PlasticGreen", PlasticGreen}, {"RubberBlack", RubberBlack}, {"Concrete", Concrete},
        {"WoodOak", WoodOak}, {"WoodCherry", WoodCherry}, {"WoodWalnut", WoodWalnut}, {"Skin", Skin}, {"Wax", Wax}, {"Jade", Jade},
        {"OilSlick", OilSlick}};
    const std::pair<const char *, Material (*)(const vec3 &)> coloured[] = {
        {"CarPaint", CarPaint}, {"PearlescentPaint", PearlescentPaint}, {"Velvet", Velvet}, {"Silk", Silk}, {"Cotton", Cotton},
        {"NeonLight", NeonLight}};
    const std::pair<const char *, Material (*)(bool)> stones[] = {
        {"MarbleCarrara", MarbleCarrara}, {"MarbleNero", MarbleNero}, {"MarbleVerde", MarbleVerde}};
    for (const auto &p : plain)
        if (n == p.first) {
            from_mat(p.second(), out);
            return 0;
        }
    for (const auto &p : coloured)
        if (n == p.first) {
            from_mat(p.second(c), out);
            return 0;
        }
    for (const auto &p : stones)
        if (n == p.first) {
            from_mat(p.second(pol), out);
            return 0;
        }
    if (n == "EmissiveLamp") {
        from_mat(EmissiveLamp(c, arg), out);
        return 0;
    }
    g_err = "hrt_material_preset: no preset " + n;
    return -1;
}

// Scenes::createLitTestScene: a new scene handle (NULL on failure)
Scene *hrt_create_lit_test_scene(int w, int h, int device) {
    try {
        Scene *s = Scenes::createLitTestScene(w, h, device).release();
        std::lock_guard<std::mutex> lock(g_mu);
        g_scenes.insert(s);
        return s;
    } catch (const std::exception &e) {
        g_err = std::string("hrt_create_lit_test_scene: ") + e.what();
        return nullptr;
    }
}

int hrt_add_cube(Scene *s, const ptrt_rt_material *m) {
    return guard(s, "addCube", [&](Scene &S) { S.addCube(to_mat(m)); return (int)S.getMeshCount() - 1; });
}
int hrt_add_plane_xz(Scene *s, float y, float half, const ptrt_rt_material *m) {
    return guard(s, "addPlaneXZ", [&](Scene &S) { S.addPlaneXZ(y, half, to_mat(m)); return (int)S.getMeshCount() - 1; });
}
int hrt_add_sphere(Scene *s, int segments, const ptrt_rt_material *m) {
    return guard(s, "addSphere", [&](Scene &S) { S.addSphere(segments, to_mat(m)); return (int)S.getMeshCount() - 1; });
}
int hrt_add_mesh(Scene *s, const char *path, const ptrt_rt_material *m) {
    return guard(s, "addMesh", [&](Scene &S) { S.addMesh(path, to_mat(m)); return (int)S.getMeshCount() - 1; }, {path});
}
int hrt_add_triangles(Scene *s, const float *corners, int n_tris, const ptrt_rt_material *m) {
    return guard(s, "addTriangles", [&](Scene &S) {
        std::vector<vec3> c;
        for (int i = 0; i < 3 * n_tris; ++i)
            c.push_back(v3(corners + 3 * i));
        S.addTriangles(c, to_mat(m));
        return (int)S.getMeshCount() - 1;
    }, {corners});
}
int hrt_add_checkerboard_plane_xz(Scene *s, float y, int tiles, float size, const ptrt_rt_material *w, const ptrt_rt_material *b) {
    return guard(s, "addCheckerboardPlaneXZ", [&](Scene &S) { S.addCheckerboardPlaneXZ(y, tiles, size, to_mat(w), to_mat(b)); return 0; });
}
int hrt_set_mesh_material(Scene *s, int i, const ptrt_rt_material *m) {
    return guard(s, "setMeshMaterial", [&](Scene &S) { S.setMeshMaterial((size_t)i, to_mat(m)); return 0; });
}
int hrt_get_mesh_material(Scene *s, int i, ptrt_rt_material *out) {
    return guard(s, "getMeshMaterial", [&](Scene &S) { from_mat(S.getMeshMaterial((size_t)i), out); return 0; }, {out});
}
int hrt_set_bvh_leaf_target(Scene *s, int target, int tol) {
    return guard(s, "setBVHLeafTarget", [&](Scene &S) { S.setBVHLeafTarget(target, tol); return 0; });
}

// Mesh methods
int hrt_mesh_scale(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::scale", [&](Scene &, Mesh &m) { m.scale(v3(f)); return 0; }, {f});
}
int hrt_mesh_translate(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::translate", [&](Scene &, Mesh &m) { m.translate(v3(f)); return 0; }, {f});
}
int hrt_mesh_move_to(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::moveTo", [&](Scene &, Mesh &m) { m.moveTo(v3(f)); return 0; }, {f});
}
int hrt_mesh_rotate_self(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::rotateSelfEulerXYZ", [&](Scene &, Mesh &m) { m.rotateSelfEulerXYZ(v3(f)); return 0; }, {f});
}
int hrt_mesh_set_position(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::setPosition", [&](Scene &, Mesh &m) { m.setPosition(v3(f)); return 0; }, {f});
}
int hrt_mesh_set_rotation(Scene *s, int i, const float *f) {
    return guard_mesh(s, i, "Mesh::setRotation", [&](Scene &, Mesh &m) { m.setRotation(v3(f)); return 0; }, {f});
}
int hrt_mesh_set_leaf_params(Scene *s, int i, int target, int tol) {
    return guard_mesh(s, i, "Mesh::setBVHLeafParams", [&](Scene &, Mesh &m) { m.setBVHLeafParams(target, tol); return 0; });
}
// a direct write of Mesh::vertices (same count), bvhDirty left as it is
int hrt_mesh_write_vertices(Scene *s, int i, const float *xyz, int n) {
    return guard_mesh(s, i, "Mesh::vertices", [&](Scene &, Mesh &m) {
        if (n != (int)m.vertices.size())
            throw std::runtime_error("vertex count differs");
        for (int k = 0; k < n; ++k)
            m.vertices[k] = v3(xyz + 3 * k);
        return 0;
    }, {xyz});
}
// counts: vertices, faces, nodes, primitives, bvhDirty
int hrt_mesh_info(Scene *s, int i, int *out5) {
    return guard_mesh(s, i, "Mesh", [&](Scene &, Mesh &m) {
        out5[0] = (int)m.vertices.size();
        out5[1] = (int)m.faces.size();
        out5[2] = (int)m.bvhNodes.size();
        out5[3] = (int)m.bvhPrimIndices.size();
        out5[4] = m.bvhDirty ? 1 : 0;
        return 0;
    }, {out5});
}
// the mesh's current arrays (any pointer may be NULL)
int hrt_mesh_read(Scene *s, int i, float *verts, int *faces, ptrt_bvh_node *nodes, int *prims) {
    return guard_mesh(s, i, "Mesh", [&](Scene &, Mesh &m) {
        if (verts && !m.vertices.empty())
            std::memcpy(verts, m.vertices.data(), m.vertices.size() * sizeof(vec3));
        if (faces && !m.faces.empty())
            std::memcpy(faces, m.faces.data(), m.faces.size() * sizeof(Tri));
        if (nodes && !m.bvhNodes.empty())
            std::memcpy(nodes, m.bvhNodes.data(), m.bvhNodes.size() * sizeof(DeviceBVHNode));
        if (prims && !m.bvhPrimIndices.empty())
            std::memcpy(prims, m.bvhPrimIndices.data(), m.bvhPrimIndices.size() * sizeof(int));
        return 0;
    });
}
int hrt_mesh_build_bvh(Scene *s, int i) {
    return guard_mesh(s, i, "Mesh::buildBVH", [&](Scene &, Mesh &m) { m.buildBVH(); return 0; });
}

// lights, sky, camera
int hrt_add_point_light(Scene *s, const float *pos, const float *col, float intensity, float range) {
    return guard(s, "addPointLight", [&](Scene &S) { S.addPointLight(v3(pos), v3(col), intensity, range); return 0; }, {pos, col});
}
int hrt_add_directional_light(Scene *s, const float *dir, const float *col, float intensity) {
    return guard(s, "addDirectionalLight", [&](Scene &S) { S.addDirectionalLight(v3(dir), v3(col), intensity); return 0; }, {dir, col});
}
int hrt_add_spot_light(Scene *s, const float *pos, const float *dir, const float *col, float intensity, float inner, float outer,
                       float range) {
    return guard(s, "addSpotLight", [&](Scene &S) { S.addSpotLight(v3(pos), v3(dir), v3(col), intensity, inner, outer, range); return 0; }, {pos, dir, col});
}
int hrt_get_light(Scene *s, int i, ptrt_rt_light *out) {
    return guard(s, "getLight", [&](Scene &S) {
        const Light &l = S.getLight((size_t)i);
        *out = ptrt_rt_light{(int32_t)l.type, pv(l.position), pv(l.direction), pv(l.color), l.intensity, l.range, l.innerCone, l.outerCone};
        return 0;
    }, {out});
}
int hrt_set_ambient_light(Scene *s, const float *a) {
    return guard(s, "setAmbientLight", [&](Scene &S) { S.setAmbientLight(v3(a)); return 0; }, {a});
}
int hrt_set_sky_gradient(Scene *s, const float *top, const float *bottom) {
    return guard(s, "setSkyGradient", [&](Scene &S) { S.setSkyGradient(v3(top), v3(bottom)); return 0; }, {top, bottom});
}
int hrt_disable_sky(Scene *s) {
    return guard(s, "disableSky", [&](Scene &S) { S.disableSky(); return 0; });
}
int hrt_set_camera(Scene *s, const float *from, const float *at, const float *up, float vfov, float aperture, float focus) {
    return guard(s, "setCamera", [&](Scene &S) { S.setCamera(v3(from), v3(at), v3(up), vfov, aperture, focus); return 0; }, {from, at, up});
}
int hrt_set_camera_simple(Scene *s, float vh, float fl) {
    return guard(s, "setCameraSimple", [&](Scene &S) { S.setCameraSimple(vh, fl); return 0; });
}
int hrt_move_camera(Scene *s, const float *p) {
    return guard(s, "moveCamera", [&](Scene &S) { S.moveCamera(v3(p)); return 0; }, {p});
}
int hrt_look_camera_at(Scene *s, const float *t, const float *up) {
    return guard(s, "lookCameraAt", [&](Scene &S) { S.lookCameraAt(v3(t), v3(up)); return 0; }, {t, up});
}
// origin, lower_left_corner, horizontal, vertical, corner_minus_origin (15 floats), lens_radius, cameraForward (3)
int hrt_get_camera(Scene *s, float *out19) {
    return guard(s, "getCamera", [&](Scene &S) {
        Camera &c = S.getCamera();
        const vec3 v[5] = {c.get_origin(), c.get_lower_left_corner(), c.get_horizontal(), c.get_vertical(), c.get_corner_minus_origin()};
        for (int k = 0; k < 5; ++k)
            for (int j = 0; j < 3; ++j)
                out19[3 * k + j] = v[k][j];
        out19[15] = c.get_lens_radius();
        const vec3 f = S.cameraForward();
        out19[16] = f.x;
        out19[17] = f.y;
        out19[18] = f.z;
        return 0;
    }, {out19});
}
// counts: meshes, lights, width, height, use_sky; then ambient, sky top, sky bottom (9 floats)
int hrt_info(Scene *s, int *out5, float *out9) {
    return guard(s, "Scene", [&](Scene &S) {
        out5[0] = (int)S.getMeshCount();
        out5[1] = (int)S.getLightCount();
        out5[2] = S.getWidth();
        out5[3] = S.getHeight();
        out5[4] = S.getUseSky() ? 1 : 0;
        const vec3 v[3] = {S.getAmbientLight(), S.getSkyTop(), S.getSkyBottom()};
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 3; ++j)
                out9[3 * k + j] = v[k][j];
        return 0;
    }, {out5, out9});
}

int hrt_upload(Scene *s) {
    return guard(s, "uploadToGPU", [&](Scene &S) { S.uploadToGPU(); return 0; });
}
int hrt_render(Scene *s, unsigned char *out) {
    return guard(s, "render", [&](Scene &S) { S.render(out); return 0; }, {out});
}
int hrt_render_to_device(Scene *s, void *dev) {
    return guard(s, "render_to_device", [&](Scene &S) { S.render_to_device((unsigned char *)dev); return 0; }, {dev});
}
int hrt_save_ppm(Scene *s, const char *path, const unsigned char *pixels) {
    return guard(s, "saveAsPPM", [&](Scene &S) { S.saveAsPPM(path, pixels); return 0; }, {path, pixels});
}

// What the last upload / render sent.  hrt_snap_counts: meshes, lights, have_view; per mesh: vertices, faces, nodes, prims
int hrt_snap_counts(Scene *s, int *out3) {
    return guard(s, "snapshot", [&](Scene &S) {
        out3[0] = (int)S.sentMeshes.size();
        out3[1] = (int)S.sentLights.size();
        out3[2] = S.viewSent ? 1 : 0;
        return 0;
    }, {out3});
}
int hrt_snap_mesh(Scene *s, int i, int *out4, float *verts, int *faces, ptrt_bvh_node *nodes, int *prims, ptrt_rt_mesh *desc) {
    return guard_mesh(s, i, "snapshot", [&](Scene &S, Mesh &m) {
        if (i >= (int)S.sentMeshes.size())
            throw std::runtime_error("mesh not sent");
        out4[0] = (int)m.sentVertices.size();
        out4[1] = (int)m.sentFaces.size();
        out4[2] = (int)m.sentNodes.size();
        out4[3] = (int)m.sentPrims.size();
        if (verts && !m.sentVertices.empty())
            std::memcpy(verts, m.sentVertices.data(), m.sentVertices.size() * sizeof(vec3));
        if (faces && !m.sentFaces.empty())
            std::memcpy(faces, m.sentFaces.data(), m.sentFaces.size() * sizeof(Tri));
        if (nodes && !m.sentNodes.empty())
            std::memcpy(nodes, m.sentNodes.data(), m.sentNodes.size() * sizeof(DeviceBVHNode));
        if (prims && !m.sentPrims.empty())
            std::memcpy(prims, m.sentPrims.data(), m.sentPrims.size() * sizeof(int));
        if (desc)
            *desc = S.sentMeshes[i];
        return 0;
    }, {out4});
}
int hrt_snap_lights(Scene *s, ptrt_rt_light *out) {
    return guard(s, "snapshot", [&](Scene &S) {
        if (!S.sentLights.empty())
            std::memcpy(out, S.sentLights.data(), S.sentLights.size() * sizeof(ptrt_rt_light));
        return 0;
    }, {out});
}
int hrt_snap_view(Scene *s, ptrt_rt_view *out) {
    return guard(s, "snapshot", [&](Scene &S) { *out = S.sentView; return 0; }, {out});
}

} // extern "C"
