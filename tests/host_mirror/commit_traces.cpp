// Which back-end calls the host mirror makes: named scenarios over host/ptrt/scene.hpp linked against the recording back end
// of fake_backend.cpp, printed as JSON -- per scenario the call lines in order, a marker line with gpuDynamicCommitCount() /
// geometryUploadCount() after every step, and the digest of serialize_scene(flatten()) taken ONCE at the end (flatten() is
// itself a read that brings host structures up to date: taking it in between would change the state under test).
//
//   commit_traces                     every scenario
//   commit_traces --stop-before-shrink   the two `shrink_after_*` scenarios end before their last commit (for recording
//                                     against headers older than the Resident record, which over-read the heap there)
//   commit_traces --time N            host time of a commit: N same-size rewrites of a 20,000-triangle soup under GpuRefit
#include "ptrt/scene.hpp" // (-I <package>/host: the Makefile takes that path as HOST_INC, so any commit's headers can be traced)
#include "ptrt/serialize.hpp"

#include <cstdio>
#include <cstdlib>
#include <functional>

std::vector<std::string> &fake_backend_log();
void fake_backend_quiet(bool);
uint64_t fake_backend_digest(const void *, size_t);

namespace {
using Policy = Scene::DynamicGeometryPolicy;

// triangle k of a sheet, heights a fixed integer function of (k, phase): no libm, the same floats everywhere
std::vector<Triangle> sheet(int n, int phase) {
    std::vector<Triangle> t;
    for (int k = 0; k < n; ++k) {
        const float x = 0.1f * (float)(k % 20) - 1.0f, z = 0.1f * (float)(k / 20) - 1.0f;
        auto y = [&](int c) { return 0.01f * (float)((k * 7 + c * 3 + phase * 13) % 17); };
        t.emplace_back(vec3(x, y(0), z), vec3(x + 0.1f, y(1), z), vec3(x, y(2), z + 0.1f));
    }
    return t;
}
// what updatePTScene does to a `Triangles` mesh (PTRTtransfer.cuh:2249-2270): both arrays replaced, both flags set
void rewrite(Mesh *m, int n, int phase) {
    std::vector<vec3> v; // (fresh arrays of exactly the new size, moved in: the old ones' memory is gone, as a caller may leave it)
    std::vector<Tri> f;
    v.reserve((size_t)n * 3);
    f.reserve((size_t)n);
    for (const Triangle &t : sheet(n, phase)) {
        const int base = (int)v.size();
        v.insert(v.end(), {t.v0, t.v1, t.v2});
        f.push_back(Tri{base, base + 1, base + 2});
    }
    m->vertices = std::move(v);
    m->faces = std::move(f);
    m->bvhDirty = m->vertsDirty = true;
    m->computeLocalAABB();
}
std::vector<float> floats(int n, int phase) {
    std::vector<float> f;
    for (const Triangle &t : sheet(n, phase))
        for (const vec3 &v : {t.v0, t.v1, t.v2})
            f.insert(f.end(), {v.x, v.y, v.z});
    return f;
}

struct Rec {
    std::vector<std::string> lines;
    std::string scene;
    void step(const char *name, Scene &s) {
        std::vector<std::string> &log = fake_backend_log();
        lines.insert(lines.end(), log.begin(), log.end());
        log.clear();
        lines.push_back(std::string("== ") + name + " counts=" + std::to_string(s.gpuDynamicCommitCount()) + "," +
                        std::to_string(s.geometryUploadCount()));
    }
    void finish(Scene &s) {
        const std::vector<uint8_t> bytes = ptrt_detail::serialize_scene(s.flatten());
        step("flatten at the end", s);
        char b[64];
        std::snprintf(b, sizeof b, "%zu:%016llx", bytes.size(), (unsigned long long)fake_backend_digest(bytes.data(), bytes.size()));
        scene = b;
    }
};

constexpr int SOUP = 4, SOUP_TRIS = 48; // mesh 4 of world(): the `Triangles` mesh
// four cubes as instances and a soup; `inner`: leaves of two, so the TLAS (and every BLAS) has inner nodes
void world(Scene &s, bool inner, Policy p = Policy::HostRebuild, bool policyFirst = true) {
    if (inner)
        s.setBVHLeafTarget(2, 0);
    for (int i = 0; i < 4; ++i)
        s.addCube()->setPosition(vec3(1.5f * (float)i - 2.0f, 0.5f, 0.25f * (float)(i * i)));
    s.addTriangles(sheet(SOUP_TRIS, 0));
    s.addPointLight(vec3(0, 3, 0), vec3(1.0f), 10.0f);
    if (policyFirst)
        s.setDynamicGeometryPolicy(p);
    s.uploadToGPU();
    if (!policyFirst)
        s.setDynamicGeometryPolicy(p);
}
void edit(Scene &s, int phase) { rewrite(s.getMesh(SOUP), SOUP_TRIS, phase); }
void commit(Rec &r, Scene &s, const char *name = "commit") {
    s.commitObjectChanges();
    r.step(name, s);
}
void lag(Rec &r, Scene &s) { // a GpuRefitAll commit of a vertex edit: host trees (and a TLAS with inner nodes) now lag the device's
    edit(s, 5);
    commit(r, s, "commit (host roots now lag)");
}
void move013(Scene &s) {
    s.getMesh(0)->setPosition(vec3(-2.5f, 0.75f, 0.0f));
    s.getMesh(1)->transform.setPosition(vec3(0.0f, 1.0f, 2.0f)); // (left dirty: the other way a move is seen)
    s.getMesh(3)->setRotation(vec3(0.0f, 0.5f, 0.0f));
}

struct Scenario {
    const char *name;
    bool both; // behind a single-leaf TLAS and behind one with inner nodes
    std::function<void(Rec &, bool)> run;
};
bool g_stopBeforeShrink = false;

void shrink(Rec &r, Policy p) { // ADVICE round 4, first item: the stale mark meets a commit that rebuilds the mesh
    Scene s(64, 64);
    s.addTriangles(sheet(400, 0));
    s.setDynamicGeometryPolicy(p);
    s.uploadToGPU();
    r.step("upload", s);
    rewrite(s.getMesh(0), 400, 1);
    commit(r, s);
    rewrite(s.getMesh(0), 50, 2);
    if (g_stopBeforeShrink)
        return;
    commit(r, s, "commit (50 triangles, nothing read in between)");
    r.finish(s);
}

const Scenario SCENARIOS[] = {
    {"host_rebuild", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         r.finish(s);
     }},
    {"gpu_refit", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefit);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         edit(s, 2);
         commit(r, s);
         r.finish(s);
     }},
    {"gpu_rebuild_then_refit", true, [](Rec &r, bool inner) { // the order mark stays pending across the refit
         Scene s(64, 64);
         world(s, inner, Policy::GpuRebuild);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         s.setDynamicGeometryPolicy(Policy::GpuRefit);
         edit(s, 2);
         commit(r, s);
         r.finish(s);
     }},
    {"refit_all_vertex_edit", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         r.finish(s);
     }},
    {"refit_all_instances_moved", true, [](Rec &r, bool inner) { // meshes 0, 1 and 3: two runs of matrices
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         move013(s);
         commit(r, s);
         r.finish(s);
     }},
    {"refit_all_edit_and_move", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         edit(s, 1);
         move013(s);
         commit(r, s);
         r.finish(s);
     }},
    {"refit_instance_changes_roots_current", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         move013(s);
         s.refitInstanceChanges();
         r.step("refitInstanceChanges", s);
         r.finish(s);
     }},
    {"refit_instance_changes_roots_lag", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         lag(r, s);
         move013(s);
         s.refitInstanceChanges();
         r.step("refitInstanceChanges", s);
         r.finish(s);
     }},
    {"reorder_tlas_roots_current", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         move013(s);
         s.reorderTLAS();
         r.step("reorderTLAS", s);
         r.finish(s);
     }},
    {"reorder_tlas_roots_lag", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         lag(r, s);
         move013(s);
         s.reorderTLAS();
         r.step("reorderTLAS", s);
         s.refitInstanceChanges(); // (the order mark stays pending across a later refit)
         r.step("refitInstanceChanges", s);
         r.finish(s);
     }},
    {"reseat_tlas_after_stale_trees", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefitAll);
         r.step("upload", s);
         lag(r, s);
         s.getMesh(2)->setPosition(vec3(3.0f, 0.5f, -1.0f));
         s.reseatTLAS();
         r.step("reseatTLAS", s);
         r.finish(s);
     }},
    {"refit_object_changes", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         edit(s, 1);
         s.refitObjectChanges();
         r.step("refitObjectChanges", s);
         r.finish(s);
     }},
    {"refit_from_host", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         const std::vector<float> v = floats(SOUP_TRIS, 3);
         s.refitFromHost(SOUP, v.data());
         r.step("refitFromHost", s);
         r.finish(s);
     }},
    {"refit_from_device", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         s.refitFromDevice(SOUP, reinterpret_cast<const float *>(uintptr_t(0x1000))); // (a device address: never followed)
         r.step("refitFromDevice", s);
         r.finish(s);
     }},
    {"rebuild_object_changes_synced", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         edit(s, 1);
         s.rebuildObjectChanges(true);
         r.step("rebuildObjectChanges(true)", s);
         r.finish(s);
     }},
    {"rebuild_object_changes_lazy", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         edit(s, 1);
         s.rebuildObjectChanges(false);
         r.step("rebuildObjectChanges(false)", s);
         commit(r, s, "commit (what the next frame does)");
         r.finish(s);
     }},
    {"rebuild_from_device", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         s.rebuildFromDevice(SOUP, reinterpret_cast<const float *>(uintptr_t(0x1000)));
         r.step("rebuildFromDevice", s);
         r.finish(s);
     }},
    {"update_triangles_fewer", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner);
         r.step("upload", s);
         const std::vector<float> v = floats(30, 4);
         s.updateTriangles(SOUP, v.data(), 30);
         r.step("updateTriangles(30 of 48)", s);
         s.updateTriangles(SOUP, reinterpret_cast<const float *>(uintptr_t(0x1000)), 12, true);
         r.step("updateTriangles(12, on the device)", s);
         r.finish(s);
     }},
    {"policy_after_upload", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefit, false);
         r.step("upload, then the policy", s);
         edit(s, 1);
         commit(r, s);
         r.finish(s);
     }},
    {"fallback_fewer_triangles", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRefit);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         s.flatten();
         r.step("flatten", s);
         rewrite(s.getMesh(SOUP), 20, 2);
         commit(r, s, "commit (20 triangles)");
         rewrite(s.getMesh(SOUP), 20, 3);
         commit(r, s, "commit (20 again)");
         r.finish(s);
     }},
    {"fallback_added_mesh", true, [](Rec &r, bool inner) {
         Scene s(64, 64);
         world(s, inner, Policy::GpuRebuild);
         r.step("upload", s);
         edit(s, 1);
         commit(r, s);
         s.addCube()->scale(0.3f);
         edit(s, 2);
         commit(r, s, "commit (a new mesh)");
         edit(s, 3);
         commit(r, s);
         r.finish(s);
     }},
    {"fresh_50_triangles", false, [](Rec &r, bool) { // what shrink_after_* must end as
         Scene s(64, 64);
         s.addTriangles(sheet(50, 2));
         s.uploadToGPU();
         r.step("upload", s);
         r.finish(s);
     }},
    {"shrink_after_gpu_refit", false, [](Rec &r, bool) { shrink(r, Policy::GpuRefit); }},
    {"shrink_after_gpu_rebuild", false, [](Rec &r, bool) { shrink(r, Policy::GpuRebuild); }},
};

void print(const std::string &name, const Rec &r, bool last) {
    std::printf("  \"%s\": {\"scene\": \"%s\", \"lines\": [\n", name.c_str(), r.scene.c_str());
    for (size_t i = 0; i < r.lines.size(); ++i)
        std::printf("    \"%s\"%s\n", r.lines[i].c_str(), i + 1 < r.lines.size() ? "," : "");
    std::printf("  ]}%s\n", last ? "" : ",");
}

int timeCommits(int n) {
    fake_backend_quiet(true);
    Scene s(64, 64);
    s.addTriangles(sheet(20000, 0));
    s.setDynamicGeometryPolicy(Policy::GpuRefit);
    s.uploadToGPU();
    const double h0 = s.commitHostMicros(), c0 = s.commitCompareMicros();
    for (int k = 1; k <= n; ++k) {
        rewrite(s.getMesh(0), 20000, k);
        s.commitObjectChanges();
    }
    if (s.gpuDynamicCommitCount() != (size_t)n || s.geometryUploadCount() != 1)
        return 1;
    std::printf("{\"commits\": %d, \"commit_host_us\": %.2f, \"compare_us\": %.2f}\n", n, (s.commitHostMicros() - h0) / n,
                (s.commitCompareMicros() - c0) / n);
    return 0;
}
} // namespace

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--time" && i + 1 < argc)
            return timeCommits(std::atoi(argv[i + 1]));
        if (a == "--stop-before-shrink")
            g_stopBeforeShrink = true;
        else {
            std::fprintf(stderr, "usage: commit_traces [--stop-before-shrink | --time N]\n");
            return 2;
        }
    }
    std::vector<std::pair<std::string, Rec>> out;
    for (const Scenario &sc : SCENARIOS)
        for (int inner = 0; inner <= (sc.both ? 1 : 0); ++inner) {
            Rec r;
            sc.run(r, inner != 0);
            fake_backend_log().clear(); // (the Scene's destructor)
            out.emplace_back(std::string(sc.name) + (sc.both ? (inner ? "/inner_nodes" : "/single_leaf") : ""), std::move(r));
        }
    std::printf("{\n");
    for (size_t i = 0; i < out.size(); ++i)
        print(out[i].first, out[i].second, i + 1 == out.size());
    std::printf("}\n");
    return 0;
}
