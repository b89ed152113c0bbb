// ptrt_query.hip.h -- the device queries of the C ABI: closest hit and occlusion (ptrt_trace_rays, ptrt_query_rays), path-traced
// radiance (ptrt_query_radiance), light probes (ptrt_query_probes), lightmap texels (ptrt_query_irradiance, with
// ptrt_irradiance_rays for the rays alone; ptrt_query_direct, with ptrt_direct_rays, for the analytic lights; ptrt_query_bounce, with
// ptrt_bounce_terms, for their one-bounce term), the lightmap
// atlas around them (ptrt_atlas_texels, ptrt_atlas_filter, ptrt_atlas_dilate: no traversal), the baked atlas read back at ray hits
// (ptrt_atlas_sample; ptrt_query_lightmap, which traces the rays itself), a probe volume read at surface points (ptrt_probe_sample;
// ptrt_query_probe_light, which traces the rays itself) and the two kernels that let a caller start where a frame starts (ptrt_camera_rays,
// ptrt_init_rng_states).  What the traversing queries share is decided once each: the traversal
// (plan_query), the kernel variant of it (with_variant, with_full), the persistent grid (launch_persistent) and the texel bakes'
// units of it (texel_groups), the refusals (check_spans, spans_apart, check_out_apart, check_shading_query); the calls without
// a traversal launch one thread per item (launch_per_item).  Included by ptrt_capi.hip behind ptrt_render.hip.h (pick_geom,
// pair_mode, trace_lds_bytes, refresh_tlas_heads) and the helpers every entry point shares.
#pragma once

#include <initializer_list>
#include <type_traits>

namespace {

// What a query decides about its trace.  The traversal is the path kernel's for this scene and these options (pair_mode
// without the merged mode): the (ray, mesh) pair walk wherever phases [B] / [D] use one, one ray per lane where they do not
// (DESIGN.md 3.15); the LDS is that traversal's; `full` is the material model a frame would use (plan_frame's).
struct QueryPlan {
    pt::KParams K;
    int geom = 0, pmode = 0;
    bool full = false;
    size_t lds = 0;
};
// `shading`: a query that runs the path loop, `samples` times to `max_depth` bounces.  A path frame that follows is ordered
// behind the query on the stream, as behind the wireframe view (option "pipeline"): `touched`.
int plan_query(ptrt_ctx *c, bool shading, int samples, int max_depth, QueryPlan &P) {
    P.K = make_params(c);
    if (shading) {
        P.K.spp = samples;
        P.K.max_depth = max_depth;
        // (the context's own per-pixel buffers are no business of the query's)
        P.K.rng = nullptr;
        P.K.accum = P.K.normal = P.K.depth = nullptr;
        P.K.object_id = nullptr;
        P.K.rgb8 = nullptr;
    }
    const int geom = P.geom = pick_geom(c);
    P.pmode = pair_mode(c, geom, false);
    P.full = c->mats_full || c->force_full;
    P.lds = trace_lds_bytes(c, geom, P.pmode);
    c->touched = true;
    c->query_pmode = P.pmode;
    c->pm1_lane_groups_eff = P.pmode == 1 ? P.K.pm1_groups : 0;
    c->plain_leaf_eff = (P.pmode == 1 || P.pmode == 2) ? P.K.plain_leaf : 0;
    return P.pmode == 3 ? refresh_tlas_heads(c, false) : PTRT_OK;
}

// f(GEOM, PMODE) with both as compile-time constants (std::integral_constant): the kernel variant of a traversal.  The pair
// walks do not depend on GEOM, one instantiation each; PMODE 0 goes by GEOM.  A wrong arm would pick a kernel built for another
// tree shape.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F> int with_variant(int geom, int pmode, F &&f) {
    switch (pmode ? pmode : -geom) {
    case 1: return f(int_c<0>{}, int_c<1>{});
    case 2: return f(int_c<1>{}, int_c<2>{});
    case 3: return f(int_c<2>{}, int_c<3>{});
    case 0: return f(int_c<0>{}, int_c<0>{});
    case -1: return f(int_c<1>{}, int_c<0>{});
    default: return f(int_c<2>{}, int_c<0>{});
    }
}

// f(FULL) with the material model as a compile-time constant (std::true_type / std::false_type): QueryPlan::full, or the
// context's own where a call has no plan.
template <class F> int with_full(bool full, F &&f) { return full ? f(std::true_type{}) : f(std::false_type{}); }

// A persistent grid of one-wave workgroups: about one per wave slot of the chip, and no more than there are `units` of work for
// the grid-stride loop (chunks of 64 rays, probes, or groups of texels). `honour_persist`: option "persist" (persistent waves per CU) overrides
// the occupancy the runtime reports -- the shading queries, not the ray queries (include/ptrt.h).
template <class Kernel, class... Args>
int launch_persistent(ptrt_ctx *c, Kernel kernel, size_t lds, size_t units, bool honour_persist, const Args &...args) {
    int per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, lds));
    if (honour_persist && c->persist > 0)
        per_cu = c->persist;
    const size_t slots = (size_t)(c->n_cus > 0 ? c->n_cus : 1) * (size_t)(per_cu > 0 ? per_cu : 1);
    const unsigned grid = (unsigned)(units < slots ? units : slots);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, c->stream, args...);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// One thread per item in blocks of 256, on the context's stream; the callers keep `items` at or below INT_MAX * 256, the grid's
// x extent being an int.  A path frame that follows is ordered behind it: `touched`.
template <class Kernel, class... Args> int launch_per_item(ptrt_ctx *c, Kernel kernel, size_t items, const Args &...args) {
    c->touched = true;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, c->stream, args...);
    HIP_TRY(c, hipGetLastError());
    return PTRT_OK;
}

// The persistent grid of the texel bakes: groups of 64 / w texels, w the smallest power of two >= the `per_texel` rays or terms
// of one; beyond 64 of them, one wave per texel.  The kernels' own statement of it (texel_shape, pt_query.hip.h).
size_t texel_groups(int n_texels, int per_texel) { return pt::texel_shape(n_texels, per_texel).groups; }

// Every span is `bytes` of device memory on the context's device (device_span), or the first that is not is refused by name.
// `optional`: a span whose pointer may be NULL, and is skipped then.
struct Span {
    const char *name;
    const void *p;
    size_t bytes;
    bool optional = false;
};
int check_spans(ptrt_ctx *c, const char *fn, std::initializer_list<Span> spans) {
    for (const Span &s : spans)
        if (!(s.optional && !s.p) && !device_span(c, s.p, s.bytes))
            return fail(c, PTRT_E_INVALID, "%s: %s is not %zu bytes of device memory on device %d", fn, s.name, s.bytes, c->device);
    return PTRT_OK;
}

// Whether two spans share no byte, and `out` against every span of `spans` in turn: the first it overlaps is refused by name.
bool spans_apart(const Span &a, const Span &b) {
    const uintptr_t x = (uintptr_t)a.p, y = (uintptr_t)b.p;
    return x < y ? y - x >= a.bytes : x - y >= b.bytes;
}
int check_out_apart(ptrt_ctx *c, const char *fn, const Span &out, std::initializer_list<Span> spans) {
    for (const Span &s : spans)
        if (!spans_apart(out, s))
            return fail(c, PTRT_E_INVALID, "%s: out %p (%zu bytes) overlaps %s %p (%zu bytes)", fn, out.p, out.bytes, s.name, s.p, s.bytes);
    return PTRT_OK;
}

// What a shading query asks of its path lengths (ptrt_render's range) and of the scene.  `max_distance`: the probes' distance
// clamp, refused between the two as ptrt_query_probes always has; NULL for a query without one.
int check_shading_query(ptrt_ctx *c, const char *fn, int samples, int max_depth, const float *max_distance) {
    if (samples < 1 || max_depth < 1 || samples > 32767 || max_depth > 32767)
        return fail(c, PTRT_E_INVALID, "%s: samples=%d max_depth=%d (1..32767)", fn, samples, max_depth);
    if (max_distance && (!(*max_distance > 0.0f) || !std::isfinite(*max_distance)))
        return fail(c, PTRT_E_INVALID, "%s: max_distance=%g (positive and finite)", fn, (double)*max_distance);
    if (!c->have_geometry || !c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "%s: %s not uploaded", fn, c->have_geometry ? "materials" : "geometry");
    if (c->n_materials < c->n_meshes)
        return fail(c, PTRT_E_NOT_READY, "%s: %d materials for %d meshes", fn, c->n_materials, c->n_meshes);
    return PTRT_OK;
}

// ray_query_kernel (pt_query.hip.h) over n rays in device memory, on the context's stream.
int launch_ray_query(ptrt_ctx *c, int kind, const float *o, const float *d, const float *tmax, size_t n, void *out) {
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    auto launch = [&](auto KIND) {
        return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::ray_query_kernel<G, PM, KIND>, P.lds, (n + 63) / 64, false, P.K, o, d, tmax, n, out);
        });
    };
    return kind == PTRT_QUERY_CLOSEST ? launch(int_c<pt::QUERY_CLOSEST>{}) : launch(int_c<pt::QUERY_OCCLUDED>{});
}

} // namespace

extern "C" {

int ptrt_trace_rays(ptrt_ctx *c, const float *origins, const float *directions, int n, ptrt_hit *out) {
    static_assert(sizeof(pt::HitOut) == sizeof(ptrt_hit), "HitOut must mirror ptrt_hit");
    if (!ctx_live(c) || !origins || !directions || !out || n < 0)
        return fail(c, PTRT_E_INVALID, "ptrt_trace_rays: bad argument");
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "ptrt_trace_rays: geometry not uploaded");
    if (n == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    // host staging around the CLOSEST query of ptrt_query_rays
    DeviceTemp<float> d_o, d_d;
    DeviceTemp<pt::HitOut> d_h;
    HIP_TRY(c, d_o.alloc((size_t)n * 3));
    HIP_TRY(c, d_d.alloc((size_t)n * 3));
    HIP_TRY(c, d_h.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(d_o.p, origins, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_d.p, directions, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_ray_query(c, PTRT_QUERY_CLOSEST, d_o.p, d_d.p, nullptr, (size_t)n, d_h.p))
        return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d_h.p, (size_t)n * sizeof(pt::HitOut), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PTRT_OK;
}

int ptrt_query_rays(ptrt_ctx *c, int kind, const float *origins, const float *directions, const float *tmax, int n, void *out) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_rays: bad context");
    if (kind != PTRT_QUERY_CLOSEST && kind != PTRT_QUERY_OCCLUDED)
        return fail(c, PTRT_E_INVALID, "ptrt_query_rays: kind %d (PTRT_QUERY_CLOSEST or PTRT_QUERY_OCCLUDED)", kind);
    if (n < 0 || !origins || !directions || !out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_rays: bad argument (n %d, origins %p, directions %p, out %p)", n,
                    (const void *)origins, (const void *)directions, out);
    if (kind == PTRT_QUERY_OCCLUDED && !tmax)
        return fail(c, PTRT_E_INVALID, "ptrt_query_rays: PTRT_QUERY_OCCLUDED needs tmax");
    if (kind == PTRT_QUERY_CLOSEST && tmax)
        return fail(c, PTRT_E_INVALID, "ptrt_query_rays: PTRT_QUERY_CLOSEST takes no tmax (pass NULL)");
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "ptrt_query_rays: geometry not uploaded");
    if (n == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    const size_t rays = (size_t)n;
    if (int rc = check_spans(c, "ptrt_query_rays",
                             {{"origins", origins, rays * 12}, {"directions", directions, rays * 12}, {"tmax", tmax, rays * sizeof(float), true},
                              {"out", out, rays * (kind == PTRT_QUERY_CLOSEST ? sizeof(pt::HitOut) : sizeof(int32_t))}}))
        return rc;
    return launch_ray_query(c, kind, origins, directions, tmax, rays, out);
}

int ptrt_query_radiance(ptrt_ctx *c, const float *origins, const float *directions, uint32_t *rng_states, int n, int samples,
                        int max_depth, ptrt_radiance *out) {
    static_assert(sizeof(pt::RadianceOut) == sizeof(ptrt_radiance) && sizeof(ptrt_radiance) == 32, "RadianceOut must mirror ptrt_radiance");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_radiance: bad context");
    if (n < 0 || !origins || !directions || !rng_states || !out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_radiance: bad argument (n %d, origins %p, directions %p, rng_states %p, out %p)", n,
                    (const void *)origins, (const void *)directions, (const void *)rng_states, (const void *)out);
    if (int rc = check_shading_query(c, "ptrt_query_radiance", samples, max_depth, nullptr))
        return rc;
    if (n == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    const size_t rays = (size_t)n;
    if (int rc = check_spans(c, "ptrt_query_radiance", {{"origins", origins, rays * 12}, {"directions", directions, rays * 12},
                                                        {"rng_states", rng_states, rays * 24}, {"out", out, rays * sizeof(ptrt_radiance)}}))
        return rc;
    QueryPlan P;
    if (int rc = plan_query(c, true, samples, max_depth, P))
        return rc;
    // radiance_query_kernel (pt_radiance.hip.h) over the n rays and their generator states
    pt::RadianceOut *o = reinterpret_cast<pt::RadianceOut *>(out);
    return with_full(P.full, [&](auto FULL) {
        return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::radiance_query_kernel<G, FULL, PM>, P.lds, (rays + 63) / 64, true, P.K, origins, directions,
                                     rng_states, rays, o);
        });
    });
}

int ptrt_query_probes(ptrt_ctx *c, const float *d_positions, int n_probes, const float *d_directions, int n_dirs,
                      uint32_t *d_rng_states, int samples, int max_depth, float max_distance, ptrt_probe *d_out) {
    static_assert(sizeof(pt::ProbeOut) == sizeof(ptrt_probe) && sizeof(ptrt_probe) == 128, "ProbeOut must mirror ptrt_probe");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_probes: bad context");
    if (n_probes < 0 || n_dirs < 1 || !d_positions || !d_directions || !d_rng_states || !d_out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_probes: bad argument (n_probes %d, n_dirs %d, positions %p, directions %p, rng_states %p, out %p)",
                    n_probes, n_dirs, (const void *)d_positions, (const void *)d_directions, (const void *)d_rng_states, (const void *)d_out);
    if (int rc = check_shading_query(c, "ptrt_query_probes", samples, max_depth, &max_distance))
        return rc;
    if (n_probes == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    // byte counts in size_t: n_probes * n_dirs rays is below 2^62 and fits; times 24 bytes of state it need not
    const size_t probes = (size_t)n_probes, ndirs = (size_t)n_dirs, rays = probes * ndirs;
    if (rays > SIZE_MAX / 24)
        return fail(c, PTRT_E_INVALID, "ptrt_query_probes: %d probes x %d directions: the states' byte count overflows", n_probes, n_dirs);
    if (int rc = check_spans(c, "ptrt_query_probes", {{"positions", d_positions, probes * 12}, {"directions", d_directions, ndirs * 12},
                                                      {"rng_states", d_rng_states, rays * 24}, {"out", d_out, probes * sizeof(ptrt_probe)}}))
        return rc;
    QueryPlan P;
    if (int rc = plan_query(c, true, samples, max_depth, P))
        return rc;
    // probe_query_kernel (pt_probe.hip.h): the grid strides over probes, one wave per probe
    pt::ProbeOut *o = reinterpret_cast<pt::ProbeOut *>(d_out);
    return with_full(P.full, [&](auto FULL) {
        return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::probe_query_kernel<G, FULL, PM>, P.lds, probes, true, P.K, d_positions, n_probes, d_directions,
                                     n_dirs, d_rng_states, max_distance, o);
        });
    });
}

int ptrt_irradiance_rays(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                         const float *d_phases, float offset, float *d_origins, float *d_directions) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_irradiance_rays: bad context");
    if (n_texels < 0 || n_dirs < 1 || !d_positions || !d_normals || !d_samples2 || !d_origins || !d_directions)
        return fail(c, PTRT_E_INVALID, "ptrt_irradiance_rays: bad argument (n_texels %d, n_dirs %d, positions %p, normals %p, samples2 %p, "
                                       "origins %p, directions %p)", n_texels, n_dirs, (const void *)d_positions, (const void *)d_normals,
                    (const void *)d_samples2, (const void *)d_origins, (const void *)d_directions);
    if (!std::isfinite(offset))
        return fail(c, PTRT_E_INVALID, "ptrt_irradiance_rays: offset=%g (finite)", (double)offset);
    if (n_texels == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    const size_t texels = (size_t)n_texels, ndirs = (size_t)n_dirs, rays = texels * ndirs;
    if (rays > SIZE_MAX / 24)
        return fail(c, PTRT_E_INVALID, "ptrt_irradiance_rays: %d texels x %d directions: the rays' byte count overflows", n_texels, n_dirs);
    // one thread per ray in blocks of 256: the grid's x extent is an int
    constexpr size_t MAX_RAYS = (size_t)INT_MAX * 256;
    if (rays > MAX_RAYS)
        return fail(c, PTRT_E_INVALID, "ptrt_irradiance_rays: %d texels x %d directions: more than %zu rays in one call", n_texels, n_dirs,
                    MAX_RAYS);
    if (int rc = check_spans(c, "ptrt_irradiance_rays",
                             {{"positions", d_positions, texels * 12}, {"normals", d_normals, texels * 12}, {"samples2", d_samples2, ndirs * 8},
                              {"phases", d_phases, texels * sizeof(float), true}, {"origins", d_origins, rays * 12},
                              {"directions", d_directions, rays * 12}}))
        return rc;
    // irradiance_rays_kernel (pt_irradiance.hip.h): one thread per ray
    return launch_per_item(c, pt::irradiance_rays_kernel, rays, d_positions, d_normals, rays, d_samples2, n_dirs, d_phases, offset, d_origins,
                           d_directions);
}

int ptrt_query_irradiance(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                          const float *d_phases, float offset, uint32_t *d_rng_states, int samples, int max_depth, float max_distance,
                          ptrt_irradiance *d_out) {
    static_assert(sizeof(pt::IrradianceOut) == sizeof(ptrt_irradiance) && sizeof(ptrt_irradiance) == 32,
                  "IrradianceOut must mirror ptrt_irradiance");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_irradiance: bad context");
    if (n_texels < 0 || n_dirs < 1 || !d_positions || !d_normals || !d_samples2 || !d_rng_states || !d_out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_irradiance: bad argument (n_texels %d, n_dirs %d, positions %p, normals %p, samples2 %p, "
                                       "rng_states %p, out %p)", n_texels, n_dirs, (const void *)d_positions, (const void *)d_normals,
                    (const void *)d_samples2, (const void *)d_rng_states, (const void *)d_out);
    if (!std::isfinite(offset))
        return fail(c, PTRT_E_INVALID, "ptrt_query_irradiance: offset=%g (finite)", (double)offset);
    if (int rc = check_shading_query(c, "ptrt_query_irradiance", samples, max_depth, &max_distance))
        return rc;
    if (n_texels == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    // byte counts in size_t: n_texels * n_dirs rays is below 2^62 and fits; times 24 bytes of state it need not
    const size_t texels = (size_t)n_texels, ndirs = (size_t)n_dirs, rays = texels * ndirs;
    if (rays > SIZE_MAX / 24)
        return fail(c, PTRT_E_INVALID, "ptrt_query_irradiance: %d texels x %d directions: the states' byte count overflows", n_texels, n_dirs);
    if (int rc = check_spans(c, "ptrt_query_irradiance",
                             {{"positions", d_positions, texels * 12}, {"normals", d_normals, texels * 12}, {"samples2", d_samples2, ndirs * 8},
                              {"phases", d_phases, texels * sizeof(float), true}, {"rng_states", d_rng_states, rays * 24},
                              {"out", d_out, texels * sizeof(ptrt_irradiance)}}))
        return rc;
    QueryPlan P;
    if (int rc = plan_query(c, true, samples, max_depth, P))
        return rc;
    // irradiance_query_kernel (pt_irradiance.hip.h): the grid strides over the texel groups of n_dirs rays a texel
    const size_t groups = texel_groups(n_texels, n_dirs);
    pt::IrradianceOut *o = reinterpret_cast<pt::IrradianceOut *>(d_out);
    return with_full(P.full, [&](auto FULL) {
        return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::irradiance_query_kernel<G, FULL, PM>, P.lds, groups, true, P.K, d_positions, d_normals, n_texels,
                                     d_samples2, n_dirs, d_phases, offset, d_rng_states, max_distance, o);
        });
    });
}

} // extern "C"

namespace {

// What ptrt_direct_rays and ptrt_query_direct refuse alike, and the counts they share: Q terms per texel, n_texels * Q rays.
struct DirectShape {
    size_t texels = 0, terms = 0, rays = 0;
};
int check_direct(ptrt_ctx *c, const char *fn, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2,
                 int n_shadow, float offset, int light_first, int light_count, DirectShape &S) {
    if (n_texels < 0 || n_shadow < 1 || !d_positions || !d_normals || !d_samples2)
        return fail(c, PTRT_E_INVALID, "%s: bad argument (n_texels %d, n_shadow %d, positions %p, normals %p, samples2 %p)", fn, n_texels,
                    n_shadow, (const void *)d_positions, (const void *)d_normals, (const void *)d_samples2);
    if (light_first < 0 || light_count < 0 || (long long)light_first + light_count > (long long)c->n_lights)
        return fail(c, PTRT_E_INVALID, "%s: lights %d .. %d + %d of %d uploaded", fn, light_first, light_first, light_count, c->n_lights);
    if (!std::isfinite(offset))
        return fail(c, PTRT_E_INVALID, "%s: offset=%g (finite)", fn, (double)offset);
    // counts in size_t: Q is below 2^62 and has to fit an int; n_texels * Q rays, times 12 bytes, has to fit size_t
    S.texels = (size_t)n_texels;
    S.terms = (size_t)light_count * (size_t)n_shadow;
    if (S.terms > (size_t)INT_MAX)
        return fail(c, PTRT_E_INVALID, "%s: %d lights x %d shadow samples: more than %d terms per texel", fn, light_count, n_shadow, INT_MAX);
    S.rays = S.texels * S.terms;
    if (S.rays > SIZE_MAX / 12)
        return fail(c, PTRT_E_INVALID, "%s: %d texels x %zu terms: the rays' byte count overflows", fn, n_texels, S.terms);
    return PTRT_OK;
}

} // namespace

extern "C" {

int ptrt_direct_rays(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_shadow,
                     const float *d_phases, float offset, int light_first, int light_count, float *d_origins, float *d_directions,
                     float *d_tmax, float *d_weights) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_direct_rays: bad context");
    if (!d_origins || !d_directions || !d_tmax || !d_weights)
        return fail(c, PTRT_E_INVALID, "ptrt_direct_rays: bad argument (origins %p, directions %p, tmax %p, weights %p)",
                    (const void *)d_origins, (const void *)d_directions, (const void *)d_tmax, (const void *)d_weights);
    DirectShape S;
    if (int rc = check_direct(c, "ptrt_direct_rays", d_positions, d_normals, n_texels, d_samples2, n_shadow, offset, light_first, light_count, S))
        return rc;
    // one thread per ray in blocks of 256: the grid's x extent is an int
    constexpr size_t MAX_RAYS = (size_t)INT_MAX * 256;
    if (S.rays > MAX_RAYS)
        return fail(c, PTRT_E_INVALID, "ptrt_direct_rays: %d texels x %zu terms: more than %zu rays in one call", n_texels, S.terms, MAX_RAYS);
    if (S.rays == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_direct_rays",
                             {{"positions", d_positions, S.texels * 12}, {"normals", d_normals, S.texels * 12},
                              {"samples2", d_samples2, (size_t)n_shadow * 8}, {"phases", d_phases, S.texels * sizeof(float), true},
                              {"origins", d_origins, S.rays * 12}, {"directions", d_directions, S.rays * 12},
                              {"tmax", d_tmax, S.rays * sizeof(float)}, {"weights", d_weights, S.rays * 12}}))
        return rc;
    // direct_rays_kernel (pt_direct.hip.h): one thread per ray
    return launch_per_item(c, pt::direct_rays_kernel, S.rays, c->d_lights, d_positions, d_normals, S.rays, d_samples2, n_shadow, d_phases,
                           offset, light_first, (int)S.terms, d_origins, d_directions, d_tmax, d_weights);
}

int ptrt_query_direct(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_shadow,
                      const float *d_phases, float offset, int light_first, int light_count, ptrt_direct *d_out) {
    static_assert(sizeof(pt::DirectOut) == sizeof(ptrt_direct) && sizeof(ptrt_direct) == 32, "DirectOut must mirror ptrt_direct");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_direct: bad context");
    if (!d_out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_direct: bad argument (out %p)", (const void *)d_out);
    DirectShape S;
    if (int rc = check_direct(c, "ptrt_query_direct", d_positions, d_normals, n_texels, d_samples2, n_shadow, offset, light_first, light_count, S))
        return rc;
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "ptrt_query_direct: geometry not uploaded");
    if (n_texels == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_query_direct",
                             {{"positions", d_positions, S.texels * 12}, {"normals", d_normals, S.texels * 12},
                              {"samples2", d_samples2, (size_t)n_shadow * 8}, {"phases", d_phases, S.texels * sizeof(float), true},
                              {"out", d_out, S.texels * sizeof(ptrt_direct)}}))
        return rc;
    if (S.terms == 0) { // no lights asked for: rows of zero bytes, in stream order
        c->touched = true;
        HIP_TRY(c, hipMemsetAsync(d_out, 0, S.texels * sizeof(ptrt_direct), c->stream));
        return PTRT_OK;
    }
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    // direct_query_kernel (pt_direct.hip.h): the grid strides over the texel groups of Q terms a texel
    const size_t groups = texel_groups(n_texels, (int)S.terms);
    pt::DirectOut *o = reinterpret_cast<pt::DirectOut *>(d_out);
    return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
        return launch_persistent(c, pt::direct_query_kernel<G, PM>, P.lds, groups, true, P.K, d_positions, d_normals, n_texels, d_samples2,
                                 n_shadow, d_phases, offset, light_first, (int)S.terms, o);
    });
}

} // extern "C"

namespace {

// What ptrt_bounce_terms and ptrt_query_bounce refuse alike, and the counts they share: n_texels * n_dirs gather rays, Q terms
// per ray, rays * Q rows.  `offset`: the query's; NULL for the call without one.
struct BounceShape {
    size_t texels = 0, dirs = 0, terms = 0, rays = 0, rows = 0;
};
int check_bounce(ptrt_ctx *c, const char *fn, int n_texels, int n_dirs, const float *d_shadow2, int n_shadow, const float *offset,
                 int light_first, int light_count, BounceShape &S) {
    if (n_texels < 0 || n_dirs < 1 || n_shadow < 1 || !d_shadow2)
        return fail(c, PTRT_E_INVALID, "%s: bad argument (n_texels %d, n_dirs %d, n_shadow %d, shadow2 %p)", fn, n_texels, n_dirs, n_shadow,
                    (const void *)d_shadow2);
    if (light_first < 0 || light_count < 0 || (long long)light_first + light_count > (long long)c->n_lights)
        return fail(c, PTRT_E_INVALID, "%s: lights %d .. %d + %d of %d uploaded", fn, light_first, light_first, light_count, c->n_lights);
    if (offset && !std::isfinite(*offset))
        return fail(c, PTRT_E_INVALID, "%s: offset=%g (finite)", fn, (double)*offset);
    // counts in size_t: Q and n_dirs * Q are below 2^62 and have to fit an int; the rows, times 12 bytes, have to fit size_t
    S.texels = (size_t)n_texels;
    S.dirs = (size_t)n_dirs;
    S.terms = (size_t)light_count * (size_t)n_shadow;
    if (S.terms > (size_t)INT_MAX || S.dirs * S.terms > (size_t)INT_MAX)
        return fail(c, PTRT_E_INVALID, "%s: %d directions x %d lights x %d shadow samples: more than %d terms per texel", fn, n_dirs,
                    light_count, n_shadow, INT_MAX);
    S.rays = S.texels * S.dirs; // (below 2^62)
    if (S.rays > SIZE_MAX / 64 || (S.terms && S.rays > SIZE_MAX / 12 / S.terms))
        return fail(c, PTRT_E_INVALID, "%s: %d texels x %d directions x %zu terms: a byte count overflows", fn, n_texels, n_dirs, S.terms);
    S.rows = S.rays * S.terms;
    return PTRT_OK;
}

} // namespace

extern "C" {

int ptrt_bounce_terms(ptrt_ctx *c, const ptrt_hit *d_hits, const float *d_directions, int n_texels, int n_dirs, const float *d_shadow2,
                      int n_shadow, const float *d_phases, int light_first, int light_count, float *d_origins, float *d_L, float *d_tmax,
                      float *d_values) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_bounce_terms: bad context");
    if (!d_hits || !d_directions || !d_origins || !d_L || !d_tmax || !d_values)
        return fail(c, PTRT_E_INVALID, "ptrt_bounce_terms: bad argument (hits %p, directions %p, origins %p, L %p, tmax %p, values %p)",
                    (const void *)d_hits, (const void *)d_directions, (const void *)d_origins, (const void *)d_L, (const void *)d_tmax,
                    (const void *)d_values);
    BounceShape S;
    if (int rc = check_bounce(c, "ptrt_bounce_terms", n_texels, n_dirs, d_shadow2, n_shadow, nullptr, light_first, light_count, S))
        return rc;
    // one thread per term in blocks of 256: the grid's x extent is an int
    constexpr size_t MAX_ROWS = (size_t)INT_MAX * 256;
    if (S.rows > MAX_ROWS)
        return fail(c, PTRT_E_INVALID, "ptrt_bounce_terms: %zu rays x %zu terms: more than %zu rows in one call", S.rays, S.terms, MAX_ROWS);
    if (!c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "ptrt_bounce_terms: materials not uploaded");
    if (S.rows == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_bounce_terms",
                             {{"hits", d_hits, S.rays * sizeof(ptrt_hit)}, {"directions", d_directions, S.rays * 12},
                              {"shadow2", d_shadow2, (size_t)n_shadow * 8}, {"phases", d_phases, S.texels * sizeof(float), true},
                              {"origins", d_origins, S.rows * 12}, {"L", d_L, S.rows * 12}, {"tmax", d_tmax, S.rows * sizeof(float)},
                              {"values", d_values, S.rows * 12}}))
        return rc;
    // bounce_terms_kernel (pt_bounce.hip.h): one thread per term, the material model a frame would use
    const pt::HitOut *h = reinterpret_cast<const pt::HitOut *>(d_hits);
    return with_full(c->mats_full || c->force_full, [&](auto FULL) {
        return launch_per_item(c, pt::bounce_terms_kernel<FULL>, S.rows, c->d_lights, c->d_materials, c->n_materials, h, d_directions, S.rows,
                               n_dirs, d_shadow2, n_shadow, d_phases, light_first, (int)S.terms, d_origins, d_L, d_tmax, d_values);
    });
}

int ptrt_query_bounce(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n_texels, const float *d_samples2, int n_dirs,
                      const float *d_phases, float offset, const float *d_shadow2, int n_shadow, int light_first, int light_count,
                      ptrt_bounce *d_out) {
    static_assert(sizeof(pt::BounceOut) == sizeof(ptrt_bounce) && sizeof(ptrt_bounce) == 32, "BounceOut must mirror ptrt_bounce");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_bounce: bad context");
    if (!d_positions || !d_normals || !d_samples2 || !d_out)
        return fail(c, PTRT_E_INVALID, "ptrt_query_bounce: bad argument (positions %p, normals %p, samples2 %p, out %p)",
                    (const void *)d_positions, (const void *)d_normals, (const void *)d_samples2, (const void *)d_out);
    BounceShape S;
    if (int rc = check_bounce(c, "ptrt_query_bounce", n_texels, n_dirs, d_shadow2, n_shadow, &offset, light_first, light_count, S))
        return rc;
    if (!c->have_geometry || !c->have_materials)
        return fail(c, PTRT_E_NOT_READY, "ptrt_query_bounce: %s not uploaded", c->have_geometry ? "materials" : "geometry");
    if (c->n_materials < c->n_meshes)
        return fail(c, PTRT_E_NOT_READY, "ptrt_query_bounce: %d materials for %d meshes", c->n_materials, c->n_meshes);
    if (n_texels == 0)
        return PTRT_OK;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_query_bounce",
                             {{"positions", d_positions, S.texels * 12}, {"normals", d_normals, S.texels * 12},
                              {"samples2", d_samples2, S.dirs * 8}, {"phases", d_phases, S.texels * sizeof(float), true},
                              {"shadow2", d_shadow2, (size_t)n_shadow * 8}, {"out", d_out, S.texels * sizeof(ptrt_bounce)}}))
        return rc;
    if (S.terms == 0) { // no lights asked for: rows of zero bytes, in stream order
        c->touched = true;
        HIP_TRY(c, hipMemsetAsync(d_out, 0, S.texels * sizeof(ptrt_bounce), c->stream));
        return PTRT_OK;
    }
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    // bounce_query_kernel (pt_bounce.hip.h): irradiance_query_kernel's grid, the texel groups of n_dirs rays a texel
    const size_t groups = texel_groups(n_texels, n_dirs);
    pt::BounceOut *o = reinterpret_cast<pt::BounceOut *>(d_out);
    return with_full(P.full, [&](auto FULL) {
        return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
            return launch_persistent(c, pt::bounce_query_kernel<G, FULL, PM>, P.lds, groups, true, P.K, d_positions, d_normals, n_texels,
                                     d_samples2, n_dirs, d_phases, offset, d_shadow2, n_shadow, light_first, (int)S.terms, o);
        });
    });
}

} // extern "C"

namespace {

// What ptrt_atlas_texels and ptrt_atlas_dilate ask of an atlas: at least one texel each way, at most 2^28 in all (a texel
// number fits an int with room for the kernels' index arithmetic).
constexpr long long ATLAS_MAX_TEXELS = 1ll << 28;
bool atlas_size_ok(int atlas_w, int atlas_h) { return atlas_w >= 1 && atlas_h >= 1 && (long long)atlas_w * atlas_h <= ATLAS_MAX_TEXELS; }
bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// Lanes per triangle when option "atlas_lanes" is -1, from the only estimate of a face's texels the host has (the atlas's
// texels over the mesh's faces).  Measured on an MI355X (profiles/atlas_time.json): 64 lanes were the fastest
// or tied in every bucket from 14 to 1.4 M texels per face; at 14 the call is three launch latencies under 16 and 64 alike,
// and below that a scan range has fewer texels than a wave has lanes.
int atlas_auto_lanes(long long texels, int faces) {
    const long long per_face = texels / (faces > 0 ? faces : 1);
    return per_face < 16 ? 16 : 64;
}

} // namespace

extern "C" {

int ptrt_atlas_texels(ptrt_ctx *c, int mesh_index, const float *d_uv, int atlas_w, int atlas_h, int clear, ptrt_atlas_texel *d_texels) {
    static_assert(sizeof(pt::AtlasTexel) == sizeof(ptrt_atlas_texel) && sizeof(ptrt_atlas_texel) == 32, "AtlasTexel must mirror ptrt_atlas_texel");
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_texels: bad context");
    if (!d_uv || !d_texels || !atlas_size_ok(atlas_w, atlas_h))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_texels: bad argument (uv %p, texels %p, atlas %d x %d: 1 x 1 .. 2^28 texels)",
                    (const void *)d_uv, (const void *)d_texels, atlas_w, atlas_h);
    if (!aligned16(d_texels) || ((uintptr_t)d_uv & 3u))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_texels: texels %p must be 16-byte aligned, uv %p 4-byte", (const void *)d_texels,
                    (const void *)d_uv);
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "ptrt_atlas_texels: geometry not uploaded");
    if (mesh_index < 0 || mesh_index >= c->n_meshes)
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_texels: mesh %d of %d uploaded", mesh_index, c->n_meshes);
    if (int rc = set_device(c))
        return rc;
    const size_t texels = (size_t)atlas_w * (size_t)atlas_h;
    const int faces = c->mesh_face_count[(size_t)mesh_index], slots = c->mesh_slot_count[(size_t)mesh_index];
    if (int rc = check_spans(c, "ptrt_atlas_texels", {{"uv", d_uv, (size_t)faces * 24}, {"texels", d_texels, texels * sizeof(ptrt_atlas_texel)}}))
        return rc;
    const int g = c->atlas_lanes > 0 ? c->atlas_lanes : atlas_auto_lanes((long long)texels, faces);
    const int log2g = g == 64 ? 6 : g == 16 ? 4 : g == 4 ? 2 : 0;
    c->atlas_lanes_eff = 1 << log2g;
    pt::AtlasTexel *t = reinterpret_cast<pt::AtlasTexel *>(d_texels);
    if (int rc = launch_per_item(c, pt::atlas_prime_kernel, texels, t, (uint32_t)texels, clear ? 1 : 0))
        return rc;
    if (slots <= 0)
        return PTRT_OK;
    // atlas_raster_kernel (pt_atlas.hip.h) twice over units of 64 / g leaf slots: the minimum face per texel, then -- behind
    // the kernel boundary -- the winners' records
    const size_t per = (size_t)(64 >> log2g), units = ((size_t)slots + per - 1) / per;
    const float4 *rec = c->d_mesh_recs + (size_t)mesh_index * pt::MESH_REC_F4;
    const int base = c->mesh_slot_base[(size_t)mesh_index];
    if (int rc = launch_persistent(c, pt::atlas_raster_kernel<1>, 0, units, true, (const float4 *)c->d_tris, (const int4 *)c->d_slot_face, rec,
                                   base, slots, mesh_index, d_uv, atlas_w, atlas_h, log2g, t))
        return rc;
    return launch_persistent(c, pt::atlas_raster_kernel<2>, 0, units, true, (const float4 *)c->d_tris, (const int4 *)c->d_slot_face, rec, base,
                             slots, mesh_index, d_uv, atlas_w, atlas_h, log2g, t);
}

int ptrt_atlas_dilate(ptrt_ctx *c, float *d_a, float *d_b, int atlas_w, int atlas_h, int passes) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_dilate: bad context");
    if (!d_a || !d_b || !atlas_size_ok(atlas_w, atlas_h) || passes < 1 || passes > 64)
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_dilate: bad argument (a %p, b %p, atlas %d x %d: 1 x 1 .. 2^28 texels, passes %d: 1 .. 64)",
                    (const void *)d_a, (const void *)d_b, atlas_w, atlas_h, passes);
    const size_t bytes = (size_t)atlas_w * (size_t)atlas_h * 16;
    if (!aligned16(d_a) || !aligned16(d_b) || !spans_apart({"a", d_a, bytes}, {"b", d_b, bytes}))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_dilate: a %p and b %p must be 16-byte aligned and %zu bytes apart", (const void *)d_a,
                    (const void *)d_b, bytes);
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_atlas_dilate", {{"a", d_a, bytes}, {"b", d_b, bytes}}))
        return rc;
    // atlas_dilate_kernel (pt_atlas.hip.h): a -> b -> a ..., one launch per pass
    float4 *buf[2] = {reinterpret_cast<float4 *>(d_a), reinterpret_cast<float4 *>(d_b)};
    for (int p = 0; p < passes; ++p)
        if (int rc = launch_per_item(c, pt::atlas_dilate_kernel, bytes / 16, (const float4 *)buf[p & 1], buf[(p & 1) ^ 1], atlas_w, atlas_h))
            return rc;
    return PTRT_OK;
}

} // extern "C"

namespace {

// Whether pass `step` of ptrt_atlas_filter runs the LDS-tile shape of atlas_filter_kernel (pt_atlas_filter.hip.h) when option
// "atlas_filter_tile" is -1.  The tile exists for steps 1, 2 and 4 (atlas_filter_tile_fits: at step 8 its halo no longer fits a
// workgroup's 64 KB).  Measured on an MI355X (profiles/atlas_filter_time.json): at all three steps the tile
// was the faster shape at every atlas and image timed -- 8 .. 10 against 12 .. 16 us at 256^2 (both near a launch's latency),
// 44 .. 50 against 75 .. 92 us at 1024^2, 0.59 .. 0.67 against 1.28 .. 1.40 ms at 4096^2 -- so the rule is: wherever it fits.
bool atlas_filter_tile_fits(int step) { return step == 1 || step == 2 || step == 4; }
bool atlas_filter_auto_tile(int step) { return atlas_filter_tile_fits(step); }

} // namespace

extern "C" {

int ptrt_atlas_filter(ptrt_ctx *c, const ptrt_atlas_texel *d_texels, float *d_a, float *d_b, int atlas_w, int atlas_h, int passes,
                      float sigma_distance, float sigma_plane, int normal_power) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_filter: bad context");
    if (!d_texels || !d_a || !d_b || !atlas_size_ok(atlas_w, atlas_h) || passes < 1 || passes > 8 || normal_power < 0 || normal_power > 7)
        return fail(c, PTRT_E_INVALID,
                    "ptrt_atlas_filter: bad argument (texels %p, a %p, b %p, atlas %d x %d: 1 x 1 .. 2^28 texels, passes %d: 1 .. 8, "
                    "normal_power %d: 0 .. 7)",
                    (const void *)d_texels, (const void *)d_a, (const void *)d_b, atlas_w, atlas_h, passes, normal_power);
    // the two ranges, squared in fp32 as the definition has them: one rr per pass, one pp
    float rr[8] = {};
    const float pp = sigma_plane * sigma_plane;
    bool ranges_ok = std::isfinite(sigma_distance) && std::isfinite(sigma_plane) && sigma_distance > 0.0f && sigma_plane > 0.0f &&
                     std::isfinite(pp) && pp != 0.0f;
    for (int p = 0; p < passes && ranges_ok; ++p) {
        const float r = sigma_distance * (float)(1 << p);
        rr[p] = r * r;
        ranges_ok = std::isfinite(rr[p]) && rr[p] != 0.0f;
    }
    if (!ranges_ok)
        return fail(c, PTRT_E_INVALID,
                    "ptrt_atlas_filter: sigma_distance %g, sigma_plane %g: positive and finite, with finite non-zero squares in fp32 at every "
                    "step of %d passes",
                    (double)sigma_distance, (double)sigma_plane, passes);
    const size_t texels = (size_t)atlas_w * (size_t)atlas_h, bytes = texels * 16, guide_bytes = texels * sizeof(ptrt_atlas_texel);
    const Span sa{"a", d_a, bytes}, sb{"b", d_b, bytes}, sg{"texels", d_texels, guide_bytes};
    if (!aligned16(d_a) || !aligned16(d_b) || !aligned16(d_texels))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_filter: texels %p, a %p and b %p must be 16-byte aligned", (const void *)d_texels,
                    (const void *)d_a, (const void *)d_b);
    if (!spans_apart(sa, sb) || !spans_apart(sa, sg) || !spans_apart(sb, sg))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_filter: a %p and b %p (%zu bytes each) and texels %p (%zu bytes) must not overlap",
                    (const void *)d_a, (const void *)d_b, bytes, (const void *)d_texels, guide_bytes);
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_atlas_filter", {sg, sa, sb}))
        return rc;
    c->touched = true;
    // atlas_filter_kernel (pt_atlas_filter.hip.h): a -> b -> a ..., one launch per pass, step 1 << pass
    static_assert(sizeof(pt::AtlasTexel) == sizeof(ptrt_atlas_texel), "AtlasTexel must mirror ptrt_atlas_texel");
    const pt::AtlasTexel *t = reinterpret_cast<const pt::AtlasTexel *>(d_texels);
    float4 *buf[2] = {reinterpret_cast<float4 *>(d_a), reinterpret_cast<float4 *>(d_b)};
    const auto tiles = [&](int tw, int th) { return ((size_t)atlas_w + tw - 1) / tw * (((size_t)atlas_h + th - 1) / th); };
    c->atlas_filter_tile_eff = 0;
    for (int p = 0; p < passes; ++p) {
        const int step = 1 << p;
        const bool tile = atlas_filter_tile_fits(step) && (c->atlas_filter_tile < 0 ? atlas_filter_auto_tile(step) : c->atlas_filter_tile != 0);
        const float4 *src = buf[p & 1];
        float4 *dst = buf[(p & 1) ^ 1];
        if (tile) {
            const unsigned tx = (unsigned)(((size_t)atlas_w + pt::FILTER_TILE - 1) / pt::FILTER_TILE);
            const dim3 grid((unsigned)tiles(pt::FILTER_TILE, pt::FILTER_TILE));
            if (step == 1)
                hipLaunchKernelGGL(pt::atlas_filter_kernel<1>, grid, dim3(256), 0, c->stream, t, src, dst, atlas_w, atlas_h, step, rr[p], pp,
                                   normal_power, tx);
            else if (step == 2)
                hipLaunchKernelGGL(pt::atlas_filter_kernel<2>, grid, dim3(256), 0, c->stream, t, src, dst, atlas_w, atlas_h, step, rr[p], pp,
                                   normal_power, tx);
            else
                hipLaunchKernelGGL(pt::atlas_filter_kernel<4>, grid, dim3(256), 0, c->stream, t, src, dst, atlas_w, atlas_h, step, rr[p], pp,
                                   normal_power, tx);
            ++c->atlas_filter_tile_eff;
        } else {
            const unsigned tx = (unsigned)(((size_t)atlas_w + pt::FILTER_ROW - 1) / pt::FILTER_ROW);
            hipLaunchKernelGGL(pt::atlas_filter_kernel<0>, dim3((unsigned)tiles(pt::FILTER_ROW, pt::FILTER_ROWS)), dim3(256), 0, c->stream, t, src,
                               dst, atlas_w, atlas_h, step, rr[p], pp, normal_power, tx);
        }
        HIP_TRY(c, hipGetLastError());
    }
    return PTRT_OK;
}

} // extern "C"

namespace {

// What ptrt_atlas_sample and ptrt_query_lightmap refuse alike, up to the device: the lightmap's four arguments, the output, and
// the caller's own inputs `ins` (the hit records; the rays), which d_out must not overlap either.  `done`: n == 0, nothing to do.
int check_lightmap(ptrt_ctx *c, const char *fn, int n, const float *d_charts, int n_chart_faces, const int32_t *d_chart_first,
                   const float *d_image, int atlas_w, int atlas_h, int mode, ptrt_lightmap_sample *d_out, std::initializer_list<Span> ins,
                   size_t in_align, pt::LightmapParams &L, bool &done) {
    static_assert(sizeof(pt::LightmapSample) == sizeof(ptrt_lightmap_sample) && sizeof(ptrt_lightmap_sample) == 32,
                  "LightmapSample must mirror ptrt_lightmap_sample");
    static_assert(pt::LIGHTMAP_NEAREST == PTRT_LIGHTMAP_NEAREST && pt::LIGHTMAP_BILINEAR == PTRT_LIGHTMAP_BILINEAR, "the modes");
    done = false;
    if (n < 0 || n_chart_faces < 1 || !d_charts || !d_chart_first || !d_image || !d_out || !atlas_size_ok(atlas_w, atlas_h) ||
        (mode != PTRT_LIGHTMAP_NEAREST && mode != PTRT_LIGHTMAP_BILINEAR))
        return fail(c, PTRT_E_INVALID,
                    "%s: bad argument (n %d, charts %p, n_chart_faces %d: >= 1, chart_first %p, image %p, atlas %d x %d: 1 x 1 .. 2^28 "
                    "texels, mode %d: 0 or 1, out %p)",
                    fn, n, (const void *)d_charts, n_chart_faces, (const void *)d_chart_first, (const void *)d_image, atlas_w, atlas_h, mode,
                    (const void *)d_out);
    for (const Span &s : ins)
        if (!s.p || ((uintptr_t)s.p & (in_align - 1)))
            return fail(c, PTRT_E_INVALID, "%s: %s %p must not be NULL and must be %zu-byte aligned", fn, s.name, s.p, in_align);
    if (!aligned16(d_image) || !aligned16(d_out) || ((uintptr_t)d_charts & 3u) || ((uintptr_t)d_chart_first & 3u))
        return fail(c, PTRT_E_INVALID, "%s: image %p and out %p must be 16-byte aligned, charts %p and chart_first %p 4-byte", fn,
                    (const void *)d_image, (const void *)d_out, (const void *)d_charts, (const void *)d_chart_first);
    if (!c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "%s: geometry not uploaded", fn);
    if (n == 0) {
        done = true;
        return PTRT_OK;
    }
    const Span charts{"charts", d_charts, (size_t)n_chart_faces * 24},
        chart_first{"chart_first", d_chart_first, (size_t)c->n_meshes * sizeof(int32_t)},
        image{"image", d_image, (size_t)atlas_w * (size_t)atlas_h * 16}, out{"out", d_out, (size_t)n * sizeof(ptrt_lightmap_sample)};
    if (int rc = check_out_apart(c, fn, out, {charts, chart_first, image}))
        return rc;
    if (int rc = check_out_apart(c, fn, out, ins))
        return rc;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, fn, ins))
        return rc;
    if (int rc = check_spans(c, fn, {charts, chart_first, image, out}))
        return rc;
    L.charts = d_charts;
    L.chart_first = d_chart_first;
    L.image = reinterpret_cast<const float4 *>(d_image);
    L.n_chart_faces = n_chart_faces;
    L.n_meshes = c->n_meshes;
    L.aw = atlas_w;
    L.ah = atlas_h;
    L.mode = mode;
    return PTRT_OK;
}

} // namespace

extern "C" {

int ptrt_atlas_sample(ptrt_ctx *c, const ptrt_hit *d_hits, int n, const float *d_charts, int n_chart_faces, const int32_t *d_chart_first,
                      const float *d_image, int atlas_w, int atlas_h, int mode, ptrt_lightmap_sample *d_out) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_atlas_sample: bad context");
    pt::LightmapParams L{};
    bool done = false;
    if (int rc = check_lightmap(c, "ptrt_atlas_sample", n, d_charts, n_chart_faces, d_chart_first, d_image, atlas_w, atlas_h, mode, d_out,
                                {{"hits", d_hits, (size_t)(n > 0 ? n : 0) * sizeof(ptrt_hit)}}, 16, L, done))
        return rc;
    if (done)
        return PTRT_OK;
    // atlas_sample_kernel (pt_lightmap.hip.h): one thread per record
    return launch_per_item(c, pt::atlas_sample_kernel, (size_t)n, reinterpret_cast<const float4 *>(d_hits), (size_t)n, L,
                           reinterpret_cast<float4 *>(d_out));
}

int ptrt_query_lightmap(ptrt_ctx *c, const float *d_origins, const float *d_directions, int n, const float *d_charts, int n_chart_faces,
                        const int32_t *d_chart_first, const float *d_image, int atlas_w, int atlas_h, int mode,
                        ptrt_lightmap_sample *d_out) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_lightmap: bad context");
    pt::LightmapParams L{};
    bool done = false;
    const size_t rays = (size_t)(n > 0 ? n : 0);
    if (int rc = check_lightmap(c, "ptrt_query_lightmap", n, d_charts, n_chart_faces, d_chart_first, d_image, atlas_w, atlas_h, mode, d_out,
                                {{"origins", d_origins, rays * 12}, {"directions", d_directions, rays * 12}}, 4, L, done))
        return rc;
    if (done)
        return PTRT_OK;
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    // lightmap_query_kernel (pt_lightmap.hip.h): ray_query_kernel's grid, chunks of 64 rays
    float4 *o = reinterpret_cast<float4 *>(d_out);
    return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
        return launch_persistent(c, pt::lightmap_query_kernel<G, PM>, P.lds, (rays + 63) / 64, false, P.K, d_origins, d_directions, rays, L, o);
    });
}

} // extern "C"

namespace {

// What ptrt_probe_sample and ptrt_query_probe_light refuse alike, up to the device: the volume, the probes, the mode, the bias,
// the output, and the caller's own float arrays `ins` (points and normals; the rays), which d_out must not overlap either.
// `need_geometry`: the fused entry traces.  `done`: n == 0, nothing to do.
int check_probe_volume(ptrt_ctx *c, const char *fn, int n, const ptrt_probe_volume *volume, const ptrt_probe *d_probes, int mode,
                       float normal_bias, ptrt_probe_light *d_out, std::initializer_list<Span> ins, bool need_geometry,
                       pt::ProbeVolumeParams &V, bool &done) {
    static_assert(sizeof(pt::ProbeLight) == sizeof(ptrt_probe_light) && sizeof(ptrt_probe_light) == 32,
                  "ProbeLight must mirror ptrt_probe_light");
    static_assert(sizeof(ptrt_probe) == 128 && offsetof(ptrt_probe, mean_distance) == 27 * 4 && offsetof(ptrt_probe, mean_distance_sq) == 28 * 4,
                  "probe_light reads a probe row by word");
    static_assert(pt::PROBES_TRILINEAR == PTRT_PROBES_TRILINEAR && pt::PROBES_VISIBILITY == PTRT_PROBES_VISIBILITY, "the modes");
    done = false;
    if (n < 0 || !volume || !d_probes || !d_out || (mode != PTRT_PROBES_TRILINEAR && mode != PTRT_PROBES_VISIBILITY) ||
        !(normal_bias >= 0.0f) || !std::isfinite(normal_bias))
        return fail(c, PTRT_E_INVALID, "%s: bad argument (n %d, volume %p, probes %p, mode %d: 0 or 1, normal_bias %g: >= 0 and finite, out %p)",
                    fn, n, (const void *)volume, (const void *)d_probes, mode, (double)normal_bias, (const void *)d_out);
    long long rows = 1;
    for (int a = 0; a < 3; ++a) {
        if (volume->counts[a] < 1 || !(volume->spacing[a] > 0.0f) || !std::isfinite(volume->spacing[a]) || !std::isfinite(volume->origin[a]))
            return fail(c, PTRT_E_INVALID, "%s: volume axis %d: count %d (>= 1), spacing %g (positive and finite), origin %g (finite)", fn, a,
                        volume->counts[a], (double)volume->spacing[a], (double)volume->origin[a]);
        rows *= volume->counts[a]; // each factor < 2^31 and the product so far <= 2^24: no overflow
        if (rows > (1ll << 24))
            return fail(c, PTRT_E_INVALID, "%s: a volume of %d x %d x %d probes (at most 2^24)", fn, volume->counts[0], volume->counts[1],
                        volume->counts[2]);
    }
    for (const Span &s : ins)
        if (!s.p || ((uintptr_t)s.p & 3u))
            return fail(c, PTRT_E_INVALID, "%s: %s %p must not be NULL and must be 4-byte aligned", fn, s.name, s.p);
    if (!aligned16(d_probes) || !aligned16(d_out))
        return fail(c, PTRT_E_INVALID, "%s: probes %p and out %p must be 16-byte aligned", fn, (const void *)d_probes, (const void *)d_out);
    if (need_geometry && !c->have_geometry)
        return fail(c, PTRT_E_NOT_READY, "%s: geometry not uploaded", fn);
    if (n == 0) {
        done = true;
        return PTRT_OK;
    }
    const Span probes{"probes", d_probes, (size_t)rows * sizeof(ptrt_probe)}, out{"out", d_out, (size_t)n * sizeof(ptrt_probe_light)};
    if (int rc = check_out_apart(c, fn, out, {probes}))
        return rc;
    if (int rc = check_out_apart(c, fn, out, ins))
        return rc;
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, fn, ins))
        return rc;
    if (int rc = check_spans(c, fn, {probes, out}))
        return rc;
    V.probes = reinterpret_cast<const float4 *>(d_probes);
    for (int a = 0; a < 3; ++a) {
        V.origin[a] = volume->origin[a];
        V.spacing[a] = volume->spacing[a];
        V.counts[a] = volume->counts[a];
    }
    V.mode = mode;
    V.bias = normal_bias;
    return PTRT_OK;
}

} // namespace

extern "C" {

int ptrt_probe_sample(ptrt_ctx *c, const float *d_positions, const float *d_normals, int n, const ptrt_probe_volume *volume,
                      const ptrt_probe *d_probes, int mode, float normal_bias, ptrt_probe_light *d_out) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_probe_sample: bad context");
    pt::ProbeVolumeParams V{};
    bool done = false;
    const size_t points = (size_t)(n > 0 ? n : 0);
    if (int rc = check_probe_volume(c, "ptrt_probe_sample", n, volume, d_probes, mode, normal_bias, d_out,
                                    {{"positions", d_positions, points * 12}, {"normals", d_normals, points * 12}}, false, V, done))
        return rc;
    if (done)
        return PTRT_OK;
    // probe_sample_kernel (pt_probe_sample.hip.h): one thread per point
    return launch_per_item(c, pt::probe_sample_kernel, points, d_positions, d_normals, points, V, reinterpret_cast<float4 *>(d_out));
}

int ptrt_query_probe_light(ptrt_ctx *c, const float *d_origins, const float *d_directions, int n, const ptrt_probe_volume *volume,
                           const ptrt_probe *d_probes, int mode, float normal_bias, ptrt_probe_light *d_out) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_query_probe_light: bad context");
    pt::ProbeVolumeParams V{};
    bool done = false;
    const size_t rays = (size_t)(n > 0 ? n : 0);
    if (int rc = check_probe_volume(c, "ptrt_query_probe_light", n, volume, d_probes, mode, normal_bias, d_out,
                                    {{"origins", d_origins, rays * 12}, {"directions", d_directions, rays * 12}}, true, V, done))
        return rc;
    if (done)
        return PTRT_OK;
    QueryPlan P;
    if (int rc = plan_query(c, false, 0, 0, P))
        return rc;
    // probe_light_query_kernel (pt_probe_sample.hip.h): ray_query_kernel's grid, chunks of 64 rays
    float4 *o = reinterpret_cast<float4 *>(d_out);
    return with_variant(P.geom, P.pmode, [&](auto G, auto PM) {
        return launch_persistent(c, pt::probe_light_query_kernel<G, PM>, P.lds, (rays + 63) / 64, false, P.K, d_origins, d_directions, rays, V,
                                 o);
    });
}

int ptrt_camera_rays(ptrt_ctx *c, int frame_index, int sample, float *d_origins, float *d_directions) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_camera_rays: bad context");
    if (frame_index < 0 || sample < 0 || frame_index > INT_MAX - sample)
        return fail(c, PTRT_E_INVALID, "ptrt_camera_rays: frame_index=%d sample=%d", frame_index, sample);
    if (!d_origins || !d_directions)
        return fail(c, PTRT_E_INVALID, "ptrt_camera_rays: a target is NULL");
    if (c->cam.lens_radius > 0.0f)
        return fail(c, PTRT_E_INVALID, "ptrt_camera_rays: a thin lens (lens_radius %g): the lens sample of a primary ray is drawn "
                                       "from the pixel's generator stream", (double)c->cam.lens_radius);
    if (int rc = set_device(c))
        return rc;
    pt::KParams K = make_params(c);
    K.frame_count = frame_index + sample;
    const size_t rays = (size_t)K.rows * K.width;
    if (int rc = check_spans(c, "ptrt_camera_rays", {{"d_origins", d_origins, rays * 12}, {"d_directions", d_directions, rays * 12}}))
        return rc;
    return launch_per_item(c, pt::camera_rays_kernel, rays, K, d_origins, d_directions);
}

int ptrt_init_rng_states(ptrt_ctx *c, unsigned long long seed, unsigned long long first_subsequence, int n, uint32_t *d_states) {
    if (!ctx_live(c, false))
        return fail(c, PTRT_E_INVALID, "ptrt_init_rng_states: bad context");
    if (n < 0 || !d_states)
        return fail(c, PTRT_E_INVALID, "ptrt_init_rng_states: bad argument (n %d, d_states %p)", n, (const void *)d_states);
    if (n == 0)
        return PTRT_OK;
    const unsigned long long last = first_subsequence + (unsigned long long)(n - 1);
    if (last < first_subsequence)
        return fail(c, PTRT_E_INVALID, "ptrt_init_rng_states: subsequence numbers beyond 2^64");
    if (int rc = set_device(c))
        return rc;
    if (int rc = check_spans(c, "ptrt_init_rng_states", {{"d_states", d_states, (size_t)n * 24}}))
        return rc;
    if (int rc = ensure_jump(c, last, "ptrt_init_rng_states"))
        return rc;
    const XorwowSeed s = xorwow_seed(seed);
    return launch_per_item(c, pt::rng_states_kernel, (size_t)n, d_states, (size_t)n, first_subsequence, s.d, s.v[0], s.v[1], s.v[2], s.v[3],
                           s.v[4], c->d_jump, c->n_jump);
}

} // extern "C"
