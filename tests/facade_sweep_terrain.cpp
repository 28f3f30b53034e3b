// Runtime check of the shape casts of include/physics_world.hpp against the heightmap terrain (sweepSphere, sweepCapsule, sweep with include flags and
// entity ranges) against libmi_physics.so (run by tests/test_facade_sweep_terrain.py; executing it needs a GPU, compiling/linking does not).
#include <cmath>
#include <cstdio>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static bool near(float a, float b, float tol = 1e-4f) { return std::fabs(a - b) <= tol; }
int main() {
    try {
        physics_world world(0);
        // no heightmap: the terrain bit of the default include changes nothing
        EXPECT(world.sweepSphere({3.3f, 5.f, 4.7f}, 0.5f, {0.f, -4.f, 0.f}).entity == MI_RAY_MISS);
        // one chunk of 16 m, every height 32768 of 65535, amplitude 4: a plane at h = 4 * 32768 / 65535 (just above 2)
        world.addHeightmap(1, 16.f, physics_material{0.05f, 0.8f, 1.f});
        std::vector<uint16_t> heights(129 * 129, (uint16_t)32768);
        world.setHeightmapChunk(0, 0, heights.data());
        world.updateHeightmap(vec3{0.f, 0.f, 0.f}, 4.f);
        const float h = 4.f * 32768.f / 65535.f;
        // a sphere of radius 0.5 from y = 5 down by 4: t = (5 - 0.5 - h) / 4
        auto s = world.sweepSphere({3.3f, 5.f, 4.7f}, 0.5f, {0.f, -4.f, 0.f});
        EXPECT(s.entity == MI_RAY_TERRAIN && s.collider == MI_RAY_TERRAIN && s.object_type == MI_OBJECT_STATIC_COLLIDER && s.flags == 0 && s.volume == 0);
        EXPECT(near(s.t, (4.5f - h) / 4.f) && near(s.normal[1], 1.f) && near(s.normal[0], 0.f) && near(s.point[1], h) && near(s.point[0], 3.3f) && near(s.point[2], 4.7f));
        // the ground probe: an upright capsule (segment y = 3.4 .. 4.4, radius 0.4: 1 m above the surface) cast 2 m down
        auto probe = world.sweepCapsule({8.f, h + 1.4f, 8.f}, {8.f, h + 2.4f, 8.f}, 0.4f, {0.f, -2.f, 0.f}, MI_QUERY_STATIC | MI_QUERY_TERRAIN);
        EXPECT(probe.entity == MI_RAY_TERRAIN && near(probe.t, 0.5f) && near(probe.normal[1], 1.f) && near(probe.point[1], h));
        // a cast that ends short of the plane, one without the terrain bit, one whose entity range leaves the terrain out
        EXPECT(world.sweepSphere({3.3f, 5.f, 4.7f}, 0.5f, {0.f, -2.f, 0.f}).entity == MI_RAY_MISS);
        EXPECT(world.sweepSphere({3.3f, 5.f, 4.7f}, 0.5f, {0.f, -4.f, 0.f}, MI_QUERY_RIGID_BODIES | MI_QUERY_STATIC).entity == MI_RAY_MISS);
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f; v.shape[0] = 3.3f; v.shape[1] = 5.f; v.shape[2] = 4.7f; v.shape[3] = 0.5f;
        auto ranged = world.sweep({v, v}, {vec3{0.f, -4.f, 0.f}, vec3{0.f, -4.f, 0.f}}, MI_QUERY_DEFAULT, {0u, MI_RAY_TERRAIN, 0u, 0xFFFFFFFFu});
        EXPECT(ranged[0].entity == MI_RAY_MISS && ranged[1].entity == MI_RAY_TERRAIN && ranged[1].volume == 1 && ranged[1].t == s.t);
        // a collider above the plane comes first; from below the plane the normal points down
        physics_material mat{0.1f, 0.5f, 1.f};
        trs t; t.position = {3.3f, 3.f, 4.7f};
        auto slab = world.addStaticCollider(t, {collider_component::asAABB({-1.f, -0.1f, -1.f}, {1.f, 0.1f, 1.f}, mat)});
        auto onSlab = world.sweepSphere({3.3f, 5.f, 4.7f}, 0.5f, {0.f, -4.f, 0.f});
        EXPECT(onSlab.entity == slab.id && near(onSlab.t, (4.5f - 3.1f) / 4.f));
        auto up = world.sweepSphere({10.f, -1.f, 10.f}, 0.5f, {0.f, 4.f, 0.f});
        EXPECT(up.entity == MI_RAY_TERRAIN && near(up.t, (h + 0.5f) / 4.f) && near(up.normal[1], -1.f));
        std::printf("facade sweep terrain ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
