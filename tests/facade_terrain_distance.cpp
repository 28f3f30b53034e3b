// Runtime check of the terrain distance queries of include/physics_world.hpp (terrainDistance, terrainClearanceOfSphere, distanceWithTerrain) against
// libmi_physics.so (run by tests/test_facade_terrain_distance.py; executing it needs a GPU, compiling/linking does not).
#include <cmath>
#include <cstdio>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static bool near(float a, float b, float tol = 1e-4f) { return std::fabs(a - b) <= tol; }
int main() {
    try {
        physics_world world(0);
        // no heightmap: a miss, and the merging call leaves the colliders' records alone
        EXPECT(world.terrainClearanceOfSphere({3.3f, 5.f, 4.7f}, 0.5f).entity == MI_RAY_MISS);
        // one chunk of 16 m, every height 32768 of 65535, amplitude 4: a plane at h = 4 * 32768 / 65535 (just above 2)
        world.addHeightmap(1, 16.f, physics_material{0.05f, 0.8f, 1.f});
        std::vector<uint16_t> heights(129 * 129, (uint16_t)32768);
        world.setHeightmapChunk(0, 0, heights.data());
        world.updateHeightmap(vec3{0.f, 0.f, 0.f}, 4.f);
        const float h = 4.f * 32768.f / 65535.f;
        // a sphere of radius 0.5 at y = 5: 4.5 - h above the plane
        auto s = world.terrainClearanceOfSphere({3.3f, 5.f, 4.7f}, 0.5f);
        EXPECT(s.entity == MI_RAY_TERRAIN && s.collider == MI_RAY_TERRAIN && s.object_type == MI_OBJECT_STATIC_COLLIDER && s.flags == 0 && s.volume == 0);
        EXPECT(near(s.distance, 4.5f - h) && near(s.normal[1], 1.f) && near(s.normal[0], 0.f) && near(s.point_collider[1], h) && near(s.point_collider[0], 3.3f) &&
               near(s.point_collider[2], 4.7f) && near(s.point_volume[1], 4.5f));
        // a maximum distance just short is a miss, just enough a hit
        EXPECT(world.terrainClearanceOfSphere({3.3f, 5.f, 4.7f}, 0.5f, 4.4f - h).entity == MI_RAY_MISS);
        EXPECT(world.terrainClearanceOfSphere({3.3f, 5.f, 4.7f}, 0.5f, 4.6f - h).entity == MI_RAY_TERRAIN);
        // below the plane the normal points down; resting in the plane is an overlap
        auto below = world.terrainClearanceOfSphere({10.f, -1.f, 10.f}, 0.5f);
        EXPECT(below.entity == MI_RAY_TERRAIN && near(below.distance, h + 0.5f) && near(below.normal[1], -1.f));
        auto in = world.terrainClearanceOfSphere({10.f, h + 0.2f, 10.f}, 0.5f);
        EXPECT(in.entity == MI_RAY_TERRAIN && in.distance == 0.f && (in.flags & MI_DISTANCE_OVERLAP) && in.normal[1] == 0.f && in.point_collider[0] == 0.f && in.point_volume[1] == 0.f);   // (the pose position: the centre is in the shape words)
        // batches
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f; v.shape[0] = 3.3f; v.shape[1] = 5.f; v.shape[2] = 4.7f; v.shape[3] = 0.5f;
        auto r = world.terrainDistance({v, v, v}, {10.f, 1.f, -1.f});
        EXPECT(r.size() == 3 && r[0].entity == MI_RAY_TERRAIN && r[0].distance == s.distance && r[1].entity == MI_RAY_MISS && r[2].entity == MI_RAY_MISS && r[2].volume == 2);
        EXPECT(world.terrainDistance({}).empty());
        bool threw = false;
        try { world.terrainDistance({v}, {1.f, 2.f}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        // the nearest of anything: a slab 1.4 under the sphere wins over the terrain, a slab far away does not
        EXPECT(world.distanceWithTerrain({v})[0].entity == MI_RAY_TERRAIN);
        physics_material mat{0.1f, 0.5f, 1.f};
        trs t; t.position = {12.f, 3.f, 12.f};
        auto far = world.addStaticCollider(t, {collider_component::asAABB({-1.f, -0.1f, -1.f}, {1.f, 0.1f, 1.f}, mat)});
        auto both = world.distanceWithTerrain({v});
        EXPECT(both[0].entity == MI_RAY_TERRAIN && both[0].distance == s.distance && world.distance({v})[0].entity == far.id);
        t.position = {3.3f, 3.f, 4.7f};
        auto slab = world.addStaticCollider(t, {collider_component::asAABB({-1.f, -0.1f, -1.f}, {1.f, 0.1f, 1.f}, mat)});
        both = world.distanceWithTerrain({v, v}, {10.f, 1.f});
        EXPECT(both[0].entity == slab.id && near(both[0].distance, 1.4f) && both[1].entity == MI_RAY_MISS && both[1].volume == 1);
        std::printf("facade terrain distance ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
