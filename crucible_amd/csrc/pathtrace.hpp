// pathtrace.hpp -- the gfx950 path-tracing megakernel and the math it shares with
// the host-side camera set-up.  Hand-written for CDNA4: wave64, one persistent
// launch, scene staged in LDS when it fits, stackless fixed-order BVH walk,
// ballot/prefix regeneration of finished lanes.  No MFMA (branchy traversal).
//
// The code lives in layered headers, included below in the order their text had in this file:
//   hd.hpp          CR_HD, CR_D
//   records.hpp     host and device: scalars, V3, Color, RNG, the records, KernelArgs, timeline, camera frame
//   intersect.hpp   device: box, sphere and triangle tests, counters
//   shade.hpp       device: trigonometry, samplers, camera rays, shade
//   walk.hpp        device: WalkState, walk_begin, walk_round
//   megakernel.hpp  device: stage_scene, pathtrace_body, the kernels
//
// Reference semantics (citations relative to the Crucible tree):
//   Camera::cast_ray / ray_color / average_samples   src/camera/ray_casting.rs:64-173
//   viewport + basis math                            src/camera/rendering_compute.rs
//   BVHWrapper::hit, Aabb::hit                       src/objects/bvhwrapper.rs:96-126, bvh.rs:96-132
//   Sphere::hit, Triangle::hit                       src/objects/sphere.rs:60-105, triangle.rs:84-140
//   Materials::scatter                               src/materials/{lambertian,metal,dielectric}.rs
//   Textures::value, SkyboxImage::get_color          src/textures/*.rs, src/scene/mod.rs:37-45
//   Point3 / Color / Interval arithmetic             src/utils.rs:78-697
// Every expression keeps the reference's operand order; the build uses
// -ffp-contract=off so no FMA is formed, and IEEE div/sqrt.
#pragma once
#include "hd.hpp"
#include "records.hpp"
#include "intersect.hpp"
#include "shade.hpp"
#include "walk.hpp"
#include "megakernel.hpp"
