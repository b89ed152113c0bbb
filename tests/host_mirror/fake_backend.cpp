// A recording stand-in for the C ABI of include/ptrt.h, for CPU tests of the host mirror (host/ptrt/scene.hpp).
//
// It defines every ptrt_* entry the mirror references and models NO geometry, no device and no frame: every call succeeds
// and appends one line to a log -- the entry's name, its scalar arguments, and for every HOST array handed in its element
// count and the 64-bit FNV-1a digest of all its bytes (reading every byte is the point: a dangling or short array shows up
// under a sanitizer).  A pointer passed with on_device = 1, and every argument the ABI documents as device memory, is
// logged as a flag and never followed.
//
// Read-backs are a fixed function of what was handed over, so a trace is reproducible:
//   ptrt_read_prim_order(mesh)  the prim order uploaded for that mesh, reversed once per ptrt_build_bvh(mesh) since;
//   ptrt_read_bvh(mesh)         the nodes uploaded for that mesh (no refit is modelled);
//   ptrt_read_tlas              the TLAS nodes last handed over (ptrt_upload_geometry / ptrt_update_instances);
//   ptrt_read_tlas_order        the TLAS mesh indices last handed over, reversed once per ptrt_reorder_tlas since.
// `fake_backend_quiet(true)` switches log and digests off (timing runs).
#include "../../include/ptrt.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

struct ptrt_ctx {
    std::vector<std::vector<int32_t>> primOrder;
    std::vector<std::vector<ptrt_bvh_node>> meshNodes;
    std::vector<ptrt_bvh_node> tlasNodes;
    std::vector<int32_t> tlasOrder;
};

static std::vector<std::string> g_log;
static bool g_quiet = false;
std::vector<std::string> &fake_backend_log() { return g_log; }
void fake_backend_quiet(bool q) { g_quiet = q; }
uint64_t fake_backend_digest(const void *p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i)
        h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

namespace {
struct Line {
    std::string s;
    explicit Line(const char *name) : s(name) {}
    Line &i(const char *k, long long v) {
        if (!g_quiet)
            s += std::string(" ") + k + "=" + std::to_string(v);
        return *this;
    }
    Line &f(const char *k, float v) {
        char b[48];
        if (!g_quiet)
            std::snprintf(b, sizeof b, " %s=%.9g", k, (double)v), s += b;
        return *this;
    }
    // a host array: count and digest; NULL is logged as such
    Line &a(const char *k, const void *p, size_t count, size_t elem) {
        if (g_quiet)
            return *this;
        char b[96];
        if (!p)
            std::snprintf(b, sizeof b, " %s=null", k);
        else
            std::snprintf(b, sizeof b, " %s[%zu]=%016llx", k, count, (unsigned long long)fake_backend_digest(p, count * elem));
        s += b;
        return *this;
    }
    Line &dev(const char *k, const void *p) { return i(k, p ? 1 : 0); } // device memory: a flag, never read
    int done() {
        if (!g_quiet)
            g_log.push_back(s);
        return PTRT_OK;
    }
};
Line &meshes(Line &l, const ptrt_mesh_desc *m, int n) {
    l.i("meshes", n);
    for (int k = 0; k < n && !g_quiet; ++k) {
        const ptrt_mesh_desc &d = m[k];
        l.a("v", d.verts, (size_t)d.vert_count, sizeof(ptrt_vec3)).a("f", d.faces, (size_t)d.face_count, sizeof(ptrt_tri));
        l.a("n", d.nodes, (size_t)d.node_count, sizeof(ptrt_bvh_node)).a("p", d.prim_indices, (size_t)d.prim_count, 4);
        l.a("w", d.world, 16, 4).a("wi", d.inverse, 16, 4).a("wn", d.normal, 16, 4).i("xf", d.has_transform);
    }
    return l;
}
Line &tlas(Line &l, ptrt_ctx *c, const ptrt_bvh_node *nodes, int nn, const int32_t *idx, int ni) {
    l.a("tlas", nodes, (size_t)nn, sizeof(ptrt_bvh_node)).a("order", idx, (size_t)ni, 4);
    c->tlasNodes.assign(nodes, nodes + nn);
    c->tlasOrder.assign(idx, idx + ni);
    return l;
}
} // namespace

extern "C" {
int ptrt_create(int w, int h, int y0, int rows, int device, ptrt_ctx **out) {
    *out = new ptrt_ctx;
    return Line("ptrt_create").i("w", w).i("h", h).i("y0", y0).i("rows", rows).i("device", device).done();
}
int ptrt_create_interleaved(int w, int h, int phase, int period, int device, ptrt_ctx **out) {
    *out = new ptrt_ctx;
    return Line("ptrt_create_interleaved").i("w", w).i("h", h).i("phase", phase).i("period", period).i("device", device).done();
}
void ptrt_destroy(ptrt_ctx *c) {
    if (c)
        Line("ptrt_destroy").done();
    delete c;
}
const char *ptrt_last_error(const ptrt_ctx *) { return "fake back end: no error"; }
int ptrt_set_blue_noise(ptrt_ctx *, const float *t) { return Line("ptrt_set_blue_noise").a("table", t, PTRT_BLUE_NOISE_FLOATS, 4).done(); }
int ptrt_reset_rng(ptrt_ctx *, unsigned long long seed) { return Line("ptrt_reset_rng").i("seed", (long long)seed).done(); }

int ptrt_upload_geometry(ptrt_ctx *c, const ptrt_mesh_desc *m, int n, const ptrt_bvh_node *tn, int tnn, const int32_t *ti, int tin) {
    Line l("ptrt_upload_geometry");
    c->primOrder.resize((size_t)n);
    c->meshNodes.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        c->primOrder[(size_t)k].assign(m[k].prim_indices, m[k].prim_indices + m[k].prim_count);
        c->meshNodes[(size_t)k].assign(m[k].nodes, m[k].nodes + m[k].node_count);
    }
    return tlas(meshes(l, m, n), c, tn, tnn, ti, tin).done();
}
int ptrt_update_instances(ptrt_ctx *c, const ptrt_mesh_desc *m, int n, const ptrt_bvh_node *tn, int tnn, const int32_t *ti, int tin) {
    // (matrices and TLAS only, as the ABI says: the geometry arrays of the descriptors may be stale and are not followed)
    Line l("ptrt_update_instances");
    l.i("meshes", n);
    for (int k = 0; k < n && !g_quiet; ++k)
        l.a("w", m[k].world, 16, 4).a("wi", m[k].inverse, 16, 4).a("wn", m[k].normal, 16, 4).i("xf", m[k].has_transform);
    return tlas(l, c, tn, tnn, ti, tin).done();
}
int ptrt_upload_materials(ptrt_ctx *, const ptrt_materials *t) {
    Line l("ptrt_upload_materials");
    const size_t n = (size_t)t->count;
    l.i("count", t->count);
    for (const ptrt_vec3 *v : {t->albedo, t->specular, t->emission, t->subsurface_color, t->sheen_tint})
        l.a("v3", v, n, sizeof(ptrt_vec3));
    for (const float *f : {t->metallic, t->roughness, t->ior, t->transmission, t->transmission_roughness, t->clearcoat,
                           t->clearcoat_roughness, t->subsurface_radius, t->anisotropy, t->sheen, t->iridescence,
                           t->iridescence_thickness})
        l.a("f", f, n, 4);
    return l.done();
}
int ptrt_upload_lights(ptrt_ctx *, const ptrt_light *l, int n) { return Line("ptrt_upload_lights").a("lights", l, (size_t)n, sizeof(ptrt_light)).done(); }
int ptrt_set_camera(ptrt_ctx *, const ptrt_camera *c) { return Line("ptrt_set_camera").a("camera", c, 1, sizeof *c).done(); }
int ptrt_set_sky(ptrt_ctx *, const ptrt_vec3 *t, const ptrt_vec3 *b, int use) {
    return Line("ptrt_set_sky").a("top", t, 1, sizeof *t).a("bottom", b, 1, sizeof *b).i("use_sky", use).done();
}
int ptrt_set_env_map(ptrt_ctx *, const float *rgba, int w, int h) {
    return Line("ptrt_set_env_map").a("rgba", rgba, (size_t)w * h * 4, 4).i("w", w).i("h", h).done();
}

int ptrt_update_vertices(ptrt_ctx *, int mesh, const float *v, int n, int on_device) {
    Line l("ptrt_update_vertices");
    l.i("mesh", mesh).i("count", n).i("on_device", on_device);
    return (on_device ? l.dev("verts", v) : l.a("verts", v, (size_t)n * 3, 4)).done();
}
int ptrt_update_triangles(ptrt_ctx *, int mesh, const float *v9, int n, int on_device) {
    Line l("ptrt_update_triangles");
    l.i("mesh", mesh).i("tris", n).i("on_device", on_device);
    return (on_device ? l.dev("verts9", v9) : l.a("verts9", v9, (size_t)n * 9, 4)).done();
}
int ptrt_refit(ptrt_ctx *) { return Line("ptrt_refit").done(); }
int ptrt_build_bvh(ptrt_ctx *c, int mesh) {
    if (mesh >= 0 && (size_t)mesh < c->primOrder.size())
        std::reverse(c->primOrder[(size_t)mesh].begin(), c->primOrder[(size_t)mesh].end());
    return Line("ptrt_build_bvh").i("mesh", mesh).done();
}
int ptrt_read_prim_order(ptrt_ctx *c, int mesh, int32_t *out, int count) {
    Line l("ptrt_read_prim_order");
    l.i("mesh", mesh).i("count", count);
    const bool known = mesh >= 0 && (size_t)mesh < c->primOrder.size();
    l.i("held", known ? (long long)c->primOrder[(size_t)mesh].size() : -1);
    for (int k = 0; k < count; ++k) // (every slot of the caller's array is written: a short array is an overflow a sanitizer sees)
        out[k] = known && (size_t)k < c->primOrder[(size_t)mesh].size() ? c->primOrder[(size_t)mesh][(size_t)k] : 0;
    return l.done();
}
int ptrt_read_bvh(ptrt_ctx *c, int mesh, ptrt_bvh_node *out, int n) {
    const bool known = mesh >= 0 && (size_t)mesh < c->meshNodes.size();
    for (int k = 0; k < n; ++k)
        out[k] = known && (size_t)k < c->meshNodes[(size_t)mesh].size() ? c->meshNodes[(size_t)mesh][(size_t)k] : ptrt_bvh_node{};
    return Line("ptrt_read_bvh").i("mesh", mesh).i("count", n).i("held", known ? (long long)c->meshNodes[(size_t)mesh].size() : -1).done();
}
int ptrt_set_instance_transforms(ptrt_ctx *, int first, int count, const ptrt_instance_xform *x) {
    return Line("ptrt_set_instance_transforms").i("first", first).a("xf", x, (size_t)count, sizeof *x).done();
}
int ptrt_refit_tlas(ptrt_ctx *) { return Line("ptrt_refit_tlas").done(); }
int ptrt_reorder_tlas(ptrt_ctx *c) {
    std::reverse(c->tlasOrder.begin(), c->tlasOrder.end());
    return Line("ptrt_reorder_tlas").done();
}
int ptrt_read_tlas(ptrt_ctx *c, ptrt_bvh_node *out, int n) {
    for (int k = 0; k < n; ++k)
        out[k] = (size_t)k < c->tlasNodes.size() ? c->tlasNodes[(size_t)k] : ptrt_bvh_node{};
    return Line("ptrt_read_tlas").i("count", n).i("held", (long long)c->tlasNodes.size()).done();
}
int ptrt_read_tlas_order(ptrt_ctx *c, int32_t *out, int n) {
    for (int k = 0; k < n; ++k)
        out[k] = (size_t)k < c->tlasOrder.size() ? c->tlasOrder[(size_t)k] : 0;
    return Line("ptrt_read_tlas_order").i("count", n).i("held", (long long)c->tlasOrder.size()).done();
}

int ptrt_denoiser_enable(ptrt_ctx *, const ptrt_denoiser_settings *s) { return Line("ptrt_denoiser_enable").i("settings", s ? 1 : 0).done(); }
int ptrt_set_prev_view_proj(ptrt_ctx *, const float *m) { return Line("ptrt_set_prev_view_proj").a("m", m, 16, 4).done(); }
int ptrt_set_bloom(ptrt_ctx *, int e) { return Line("ptrt_set_bloom").i("enabled", e).done(); }
int ptrt_set_render_size(ptrt_ctx *, int w, int h) { return Line("ptrt_set_render_size").i("w", w).i("h", h).done(); }
int ptrt_set_option(ptrt_ctx *, const char *name, long long v) { return Line("ptrt_set_option").i(name, v).done(); }
int ptrt_render(ptrt_ctx *, int frame, int spp, int depth, void *out, int is_device) {
    return Line("ptrt_render").i("frame", frame).i("spp", spp).i("depth", depth).dev("out", out).i("out_is_device", is_device).done();
}
int ptrt_render_wireframe(ptrt_ctx *, float t, void *out, int is_device) {
    return Line("ptrt_render_wireframe").f("thickness", t).dev("out", out).i("out_is_device", is_device).done();
}
int ptrt_sync(ptrt_ctx *) { return Line("ptrt_sync").done(); }
void *ptrt_device_buffer(ptrt_ctx *, int kind) {
    Line("ptrt_device_buffer").i("kind", kind).done();
    return nullptr;
}
int ptrt_post_frame(ptrt_ctx *, const float *a, const float *n, const float *d, const int32_t *o, void *out, int is_device) {
    return Line("ptrt_post_frame").dev("accum", a).dev("normal", n).dev("depth", d).dev("object_id", o).dev("out", out).i("out_is_device", is_device).done();
}
int ptrt_trace_rays(ptrt_ctx *, const float *o, const float *d, int n, ptrt_hit *out) {
    std::memset(out, 0, (size_t)n * sizeof *out);
    return Line("ptrt_trace_rays").a("origins", o, (size_t)n * 3, 4).a("dirs", d, (size_t)n * 3, 4).done();
}
int ptrt_query_rays(ptrt_ctx *, int kind, const float *o, const float *d, const float *t, int n, void *out) {
    return Line("ptrt_query_rays").i("kind", kind).dev("origins", o).dev("dirs", d).dev("tmax", t).i("n", n).dev("out", out).done();
}
int ptrt_query_radiance(ptrt_ctx *, const float *o, const float *d, uint32_t *rng, int n, int samples, int depth, ptrt_radiance *out) {
    return Line("ptrt_query_radiance").dev("origins", o).dev("dirs", d).dev("rng", rng).i("n", n).i("samples", samples).i("depth", depth).dev("out", out).done();
}
int ptrt_query_probes(ptrt_ctx *, const float *p, int np, const float *d, int nd, uint32_t *rng, int samples, int depth, float maxd, ptrt_probe *out) {
    return Line("ptrt_query_probes").dev("positions", p).i("probes", np).dev("dirs", d).i("n_dirs", nd).dev("rng", rng).i("samples", samples).i("depth", depth).f("max_distance", maxd).dev("out", out).done();
}
int ptrt_irradiance_rays(ptrt_ctx *, const float *p, const float *nrm, int nt, const float *s2, int nd, const float *ph, float off, float *o, float *d) {
    return Line("ptrt_irradiance_rays").dev("positions", p).dev("normals", nrm).i("texels", nt).dev("samples2", s2).i("n_dirs", nd).dev("phases", ph).f("offset", off).dev("origins", o).dev("dirs", d).done();
}
int ptrt_query_irradiance(ptrt_ctx *, const float *p, const float *nrm, int nt, const float *s2, int nd, const float *ph, float off, uint32_t *rng, int samples, int depth, float maxd, ptrt_irradiance *out) {
    return Line("ptrt_query_irradiance").dev("positions", p).dev("normals", nrm).i("texels", nt).dev("samples2", s2).i("n_dirs", nd).dev("phases", ph).f("offset", off).dev("rng", rng).i("samples", samples).i("depth", depth).f("max_distance", maxd).dev("out", out).done();
}
int ptrt_camera_rays(ptrt_ctx *, int frame, int sample, float *o, float *d) {
    return Line("ptrt_camera_rays").i("frame", frame).i("sample", sample).dev("origins", o).dev("dirs", d).done();
}
int ptrt_init_rng_states(ptrt_ctx *, unsigned long long seed, unsigned long long first, int n, uint32_t *out) {
    return Line("ptrt_init_rng_states").i("seed", (long long)seed).i("first", (long long)first).i("n", n).dev("states", out).done();
}
} // extern "C"
