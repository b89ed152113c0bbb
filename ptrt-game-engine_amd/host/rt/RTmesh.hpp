// rt/RTmesh.hpp -- host mirror of the ray tracer's Mesh (src/raytracer/RTmesh.cuh:289-658): geometry, the
// median-split "SAH" builder, the OBJ loader and the vertex-baking transforms.  Device memory is not owned here: the
// Scene (RTscene.hpp) sends a mesh through the C ABI of include/ptrt.h and keeps what it sent.
#pragma once
#include "../ptrt/math.hpp"

#include <algorithm>
#include <cstdint>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace ptrt_rt {

struct Tri {
    int v0, v1, v2;
};

struct AABB {
    vec3 bmin, bmax;
    vec3 extent() const { return vec3(bmax.x - bmin.x, bmax.y - bmin.y, bmax.z - bmin.z); }
    vec3 center() const { return vec3((bmin.x + bmax.x) * 0.5f, (bmin.y + bmax.y) * 0.5f, (bmin.z + bmax.z) * 0.5f); }
    static AABB make_invalid() { return AABB{vec3(1e30f), vec3(-1e30f)}; }
    void expand(const vec3 &p) {
        bmin = vec3(std::fmin(bmin.x, p.x), std::fmin(bmin.y, p.y), std::fmin(bmin.z, p.z));
        bmax = vec3(std::fmax(bmax.x, p.x), std::fmax(bmax.y, p.y), std::fmax(bmax.z, p.z));
    }
    void expand(const AABB &b) {
        expand(b.bmin);
        expand(b.bmax);
    }
};

struct DeviceBVHNode { // the 40 bytes of ptrt_bvh_node
    AABB bbox;
    int left, right, start, count;
};

class Mesh {
  public:
    std::vector<vec3> vertices;
    std::vector<Tri> faces;
    vec3 position = vec3(0.0f);
    vec3 rotationEuler = vec3(0.0f);
    std::vector<DeviceBVHNode> bvhNodes;
    std::vector<int> bvhPrimIndices;
    bool bvhDirty = true;
    int bvhLeafTarget = 4;
    int bvhLeafTol = 2;

    // what the Scene last sent to the device for this mesh (empty before the first upload)
    std::vector<vec3> sentVertices;
    std::vector<Tri> sentFaces;
    std::vector<DeviceBVHNode> sentNodes;
    std::vector<int> sentPrims;
    bool sentTree = false;

    // the default mesh: a unit cube centred at (0, 0, -3) (RTmesh.cuh:375-383)
    Mesh() {
        vertices = {{-0.5f, -0.5f, -3.5f}, {0.5f, -0.5f, -3.5f}, {0.5f, 0.5f, -3.5f}, {-0.5f, 0.5f, -3.5f},
                    {-0.5f, -0.5f, -2.5f}, {0.5f, -0.5f, -2.5f}, {0.5f, 0.5f, -2.5f}, {-0.5f, 0.5f, -2.5f}};
        faces = {{0, 2, 1}, {0, 3, 2}, {4, 5, 6}, {4, 6, 7}, {0, 1, 5}, {0, 5, 4},
                 {3, 7, 6}, {3, 6, 2}, {0, 4, 7}, {0, 7, 3}, {1, 2, 6}, {1, 6, 5}};
    }
    // OBJ: `v x y z` and `f a b c ...` (1-based, `a/b/c` forms take the first index, polygons fanned); '#' lines skipped
    explicit Mesh(const std::string &path) {
        std::ifstream in(path);
        if (!in)
            throw std::runtime_error("Mesh: cannot open " + path);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#')
                continue;
            std::istringstream ss(line);
            std::string key;
            ss >> key;
            if (key == "v") {
                float x, y, z;
                ss >> x >> y >> z;
                vertices.emplace_back(x, y, z);
            } else if (key == "f") {
                std::vector<int> idx;
                std::string tok;
                while (ss >> tok)
                    idx.push_back(std::stoi(tok.substr(0, tok.find('/'))) - 1);
                for (size_t i = 1; i + 1 < idx.size(); ++i)
                    faces.push_back({idx[0], idx[i], idx[i + 1]});
            }
        }
        if (vertices.empty() || faces.empty())
            throw std::runtime_error("Mesh: no geometry in " + path);
    }

    void setPosition(const vec3 &p) { position = p; }
    void setRotation(const vec3 &r) { rotationEuler = r; }
    void setBVHLeafParams(int target, int tol = 2) {
        bvhLeafTarget = target < 1 ? 1 : target;
        bvhLeafTol = tol < 0 ? 0 : tol;
        bvhDirty = true;
    }
    size_t faceCount() const { return faces.size(); }
    size_t vertexCount() const { return vertices.size(); }

    AABB boundingBox() const {
        if (vertices.empty())
            return AABB{vec3(0.0f), vec3(0.0f)};
        AABB b{vertices[0], vertices[0]};
        for (size_t i = 1; i < vertices.size(); ++i)
            b.expand(vertices[i]);
        return b;
    }
    void scale(float s) { scale(vec3(s)); }
    void scale(vec3 s) {
        for (auto &v : vertices) {
            v.x *= s.x;
            v.y *= s.y;
            v.z *= s.z;
        }
        bvhDirty = true;
    }
    void translate(const vec3 &d) {
        for (auto &v : vertices) {
            v.x += d.x;
            v.y += d.y;
            v.z += d.z;
        }
        bvhDirty = true;
    }
    void moveTo(const vec3 &p) { translate(p - boundingBox().center()); }
    // about the bounding-box centre, X then Y then Z (RTmesh.cuh:633-656)
    void rotateSelfEulerXYZ(const vec3 &rad) {
        const vec3 c = boundingBox().center();
        const float cx = std::cos(rad.x), sx = std::sin(rad.x);
        const float cy = std::cos(rad.y), sy = std::sin(rad.y);
        const float cz = std::cos(rad.z), sz = std::sin(rad.z);
        for (auto &v : vertices) {
            vec3 p = v - c;
            p = vec3(p.x, cx * p.y - sx * p.z, sx * p.y + cx * p.z);
            p = vec3(cy * p.x + sy * p.z, p.y, -sy * p.x + cy * p.z);
            p = vec3(cz * p.x - sz * p.y, sz * p.x + cz * p.y, p.z);
            v = p + c;
        }
        bvhDirty = true;
    }

    // Mesh::buildBVH (RTmesh.cuh:465-552): nodes in pre-order; a range of at most target + tol faces is a leaf, any
    // other is split at its middle by std::nth_element on the centroid axis of largest extent
    void buildBVH() {
        bvhNodes.clear();
        bvhPrimIndices.clear();
        if (faces.empty()) {
            bvhDirty = false;
            return;
        }
        struct Ref {
            int f;
            vec3 c;
            AABB b;
        };
        std::vector<Ref> refs;
        refs.reserve(faces.size());
        for (int i = 0; i < (int)faces.size(); ++i) {
            const vec3 &a = vertices[faces[i].v0], &b = vertices[faces[i].v1], &c = vertices[faces[i].v2];
            AABB bb{vec3(std::fmin(std::fmin(a.x, b.x), c.x), std::fmin(std::fmin(a.y, b.y), c.y), std::fmin(std::fmin(a.z, b.z), c.z)),
                    vec3(std::fmax(std::fmax(a.x, b.x), c.x), std::fmax(std::fmax(a.y, b.y), c.y), std::fmax(std::fmax(a.z, b.z), c.z))};
            refs.push_back(Ref{i, (a + b + c) * (1.0f / 3.0f), bb});
        }
        const int leafMax = bvhLeafTarget + bvhLeafTol;
        struct Builder {
            std::vector<DeviceBVHNode> &nodes;
            std::vector<int> &prims;
            std::vector<Ref> &R;
            int leafMax;
            int build(int begin, int end) {
                AABB bb = AABB::make_invalid(), cb = AABB::make_invalid();
                for (int i = begin; i < end; ++i) {
                    bb.expand(R[i].b);
                    cb.expand(R[i].c);
                }
                const int n = end - begin;
                const int me = (int)nodes.size();
                nodes.push_back(DeviceBVHNode{bb, -1, -1, -1, 0});
                if (n <= leafMax) {
                    nodes[me].start = (int)prims.size();
                    nodes[me].count = n;
                    for (int i = begin; i < end; ++i)
                        prims.push_back(R[i].f);
                    return me;
                }
                const vec3 e = cb.extent();
                const int axis = (e.x > e.y && e.x > e.z) ? 0 : ((e.y > e.z) ? 1 : 2);
                const int mid = (begin + end) / 2;
                std::nth_element(R.begin() + begin, R.begin() + mid, R.begin() + end,
                                 [axis](const Ref &A, const Ref &B) { return A.c[axis] < B.c[axis]; });
                const int L = build(begin, mid);
                const int Rn = build(mid, end);
                nodes[me].left = L;
                nodes[me].right = Rn;
                return me;
            }
        };
        Builder B{bvhNodes, bvhPrimIndices, refs, leafMax};
        B.build(0, (int)refs.size());
        bvhDirty = false;
    }
};

} // namespace ptrt_rt
