// Forwarding header for callers of the reference's ray tracer: with -I <this package>/host/fwd, an unchanged
// `#include "raytracer/RTscene.cuh"` gets the host mirror (host/rt/RTscene.hpp), and its names -- Scene, Mesh,
// Material, Light, Camera, Materials::*, Scenes::* -- are in scope at global level as in the reference's own file.
// (They live in namespace ptrt_rt because the path tracer's mirror has global classes of the same names in the same
// library; a translation unit that includes both mirrors names the RT ones ptrt_rt::...)
#pragma once
#include "../../rt/RTscene.hpp"

using namespace ptrt_rt;
