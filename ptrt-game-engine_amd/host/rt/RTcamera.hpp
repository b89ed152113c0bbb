// rt/RTcamera.hpp -- host mirror of the ray tracer's Camera (src/raytracer/RTcamera.cuh).  The kernel only reads
// origin, corner_minus_origin, horizontal and vertical; the lens radius is kept for the host get_ray, as in the
// reference, whose device branch ignores it.
#pragma once
#include "../ptrt/math.hpp"

#include <cstdint>

namespace ptrt_rt {

class Camera {
    vec3 origin, lower_left_corner, horizontal, vertical, u, v, w;
    float lens_radius = 0.0f;
    vec3 corner_minus_origin;

  public:
    // look-from constructor (RTcamera.cuh:71-91)
    Camera(vec3 lookfrom, vec3 lookat, vec3 vup, float vfov, float aspect_ratio, float aperture = 0.0f,
           float focus_dist = 1.0f) {
        const float theta = vfov * 0.01745329251994329577f;
        const float h = std::tan(theta * 0.5f);
        const float viewport_height = 2.0f * h;
        const float viewport_width = aspect_ratio * viewport_height;
        w = (lookfrom - lookat).normalized();
        u = cross(vup, w).normalized();
        v = cross(w, u);
        origin = lookfrom;
        horizontal = focus_dist * viewport_width * u;
        vertical = focus_dist * viewport_height * v;
        lower_left_corner = origin - horizontal * 0.5f - vertical * 0.5f - focus_dist * w;
        corner_minus_origin = lower_left_corner - origin;
        lens_radius = aperture * 0.5f;
    }
    // simple constructor (RTcamera.cuh:93-108): `vertical` points DOWN
    explicit Camera(float aspect_ratio, float viewport_height = 2.0f, float focal_length = 1.0f) {
        origin = vec3(0.0f, 0.0f, 0.0f);
        const float viewport_width = viewport_height * aspect_ratio;
        horizontal = vec3(viewport_width, 0.0f, 0.0f);
        vertical = vec3(0.0f, -viewport_height, 0.0f);
        lower_left_corner = origin - horizontal * 0.5f - vertical * 0.5f - vec3(0.0f, 0.0f, focal_length);
        corner_minus_origin = lower_left_corner - origin;
        lens_radius = 0.0f;
        u = vec3(1, 0, 0);
        v = vec3(0, 1, 0);
        w = vec3(0, 0, 1);
    }

    vec3 get_origin() const { return origin; }
    vec3 get_lower_left_corner() const { return lower_left_corner; }
    vec3 get_horizontal() const { return horizontal; }
    vec3 get_vertical() const { return vertical; }
    vec3 get_corner_minus_origin() const { return corner_minus_origin; }
    float get_lens_radius() const { return lens_radius; }

    // RTcamera.cuh:169-176
    void set_position(const vec3 &pos) {
        const vec3 delta = pos - origin;
        origin = pos;
        lower_left_corner = lower_left_corner + delta;
        corner_minus_origin = lower_left_corner - origin;
    }
    // RTcamera.cuh:178-196: keeps the viewport's size, focuses at the target
    void look_at(const vec3 &target, const vec3 &vup = vec3(0, 1, 0)) {
        w = (origin - target).normalized();
        u = cross(vup, w).normalized();
        v = cross(w, u);
        const float viewport_height = vertical.length();
        const float viewport_width = horizontal.length();
        const float focus_dist = (origin - target).length();
        horizontal = viewport_width * u;
        vertical = viewport_height * v;
        lower_left_corner = origin - horizontal * 0.5f - vertical * 0.5f - focus_dist * w;
        corner_minus_origin = lower_left_corner - origin;
    }
};

} // namespace ptrt_rt
