// plain_leaf.h -- option "plain_leaf": is the uploaded scene one whose pair builder may leave out the TLAS root-box test and
// whose pair batches may leave out the instance arithmetic (build_pairs, closest_hit_pairs / any_hit_pairs, pt_render.hip.h;
// DESIGN.md 3.24)?  Plain C++, no HIP: the device library derives the flag at upload, the host-only entry point
// ptrt_plain_leaf derives it from the same arrays without a device.
//
// The flag is true when
//   - the TLAS root is a single leaf,
//   - no mesh of that leaf has a transform (its root test then runs on the world ray, and a pair's ray is the world ray), and
//   - the root-test box of every mesh of the leaf lies inside the TLAS root box, component by component, compared on the fp32
//     values that are uploaded.
// Why the third line makes the root test redundant: slab() (pt_kernels.hip.h) forms per axis (plane - o) * inv with the SAME o
// and inv for both boxes.  The subtraction and the multiplication by a fixed factor are monotone in `plane` under round to
// nearest, infinities included, so on every axis the mesh box's entry distance is >= the root's and its exit distance <= the
// root's; max and min keep that order, and each of the three conjuncts (tmax >= 0, tmin <= tmax, tmin < tMax) that holds for
// the inner interval holds for the outer one.  A ray that passes a mesh's test passes the root's with the same limit; a ray that
// fails the root's passes no mesh's: the pair list is the same entry for entry with and without the root test.  A NaN compares
// false here and clears the flag.
#pragma once
#include "../../include/ptrt.h"

#include <vector>

namespace pt {

// `boxes`: per mesh of the leaf six floats {bmin.xyz, bmax.xyz}, the root-test box of its mesh record; `has_transform`: per mesh
// of the leaf, non-zero for an instance; `root`: {bmin.xyz, bmax.xyz} of TLAS node 0.
inline bool plain_leaf_derive(bool tlas_single_leaf, const float *root, const float *boxes, const unsigned char *has_transform,
                              int leaf_meshes) {
    if (!tlas_single_leaf || !root || leaf_meshes < 0 || (leaf_meshes > 0 && (!boxes || !has_transform)))
        return false;
    for (int m = 0; m < leaf_meshes; ++m) {
        if (has_transform[m])
            return false;
        const float *b = boxes + 6 * m;
        for (int k = 0; k < 3; ++k)
            if (!(b[k] >= root[k]) || !(b[3 + k] <= root[3 + k]))
                return false;
    }
    return true;
}

// The same over the arrays ptrt_upload_geometry takes (a mesh's root-test box is node 0 of its BVH, as flatten_mesh records
// it).  Arrays that the upload would refuse give false.
inline bool plain_leaf_scene(const ptrt_mesh_desc *meshes, int mesh_count, const ptrt_bvh_node *tlas_nodes, int tlas_node_count,
                             const int32_t *tlas_mesh_indices, int tlas_index_count) {
    if (!meshes || mesh_count <= 0 || !tlas_nodes || tlas_node_count <= 0 || !tlas_mesh_indices || tlas_index_count <= 0)
        return false;
    const ptrt_bvh_node &R = tlas_nodes[0];
    if (R.count <= 0 || R.start < 0 || R.start > tlas_index_count - R.count) // (an inner node at the root: not a single leaf)
        return false;
    std::vector<float> boxes;
    std::vector<unsigned char> xf;
    for (int k = 0; k < R.count; ++k) {
        const int m = tlas_mesh_indices[R.start + k];
        if (m < 0 || m >= mesh_count || !meshes[m].nodes || meshes[m].node_count <= 0)
            return false;
        const ptrt_bvh_node &N = meshes[m].nodes[0];
        boxes.insert(boxes.end(), {N.bmin.x, N.bmin.y, N.bmin.z, N.bmax.x, N.bmax.y, N.bmax.z});
        xf.push_back(meshes[m].has_transform ? 1 : 0);
    }
    const float root[6] = {R.bmin.x, R.bmin.y, R.bmin.z, R.bmax.x, R.bmax.y, R.bmax.z};
    return plain_leaf_derive(true, root, boxes.data(), xf.data(), R.count);
}

} // namespace pt
