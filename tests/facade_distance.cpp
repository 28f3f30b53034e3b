// Runtime check of the distance queries of include/physics_world.hpp (distance with and without maximum distances and entity ranges,
// distanceToSphere) against libmi_physics.so (run by tests/test_facade_distance.py; executing it needs a GPU, compiling/linking does not).
#include <cmath>
#include <cstdio>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static bool near(float a, float b, float tol = 1e-4f) { return std::fabs(a - b) <= tol; }
int main() {
    try {
        physics_world world(0);
        physics_material mat{0.1f, 0.5f, 1.f};
        auto ground = world.addStaticCollider(trs{}, {collider_component::asAABB({-50, -4, -50}, {50, 0, 50}, mat)});
        trs t; t.position = {0, 2, 0};
        auto a = world.addRigidBody(t, rigid_body_component{}, {collider_component::asSphere({0, 0, 0}, 0.5f, mat)});
        t.position = {3, 2, 0};
        auto b = world.addRigidBody(t, rigid_body_component{}, {collider_component::asAABB({-0.5f, -0.5f, -0.5f}, {0.5f, 0.5f, 0.5f}, mat)});
        // a sphere of radius 0.25 at x = -2: the sphere body's surface is 2 - 0.5 - 0.25 away, the ground 2 - 0.25
        auto s = world.distanceToSphere({-2.f, 2.f, 0.f}, 0.25f);
        EXPECT(s.entity == a.id && s.object_type == MI_OBJECT_RIGID_BODY && s.flags == 0 && s.volume == 0);
        EXPECT(near(s.distance, 1.25f) && near(s.normal[0], -1.f) && near(s.normal[1], 0.f) && near(s.point_collider[0], -0.5f) && near(s.point_volume[0], -1.75f) && near(s.point_volume[1], 2.f));
        // right of the box: its face x = 3.5
        auto right = world.distanceToSphere({5.f, 2.f, 0.f}, 0.25f);
        EXPECT(right.entity == b.id && near(right.distance, 1.25f) && near(right.normal[0], 1.f) && near(right.point_collider[0], 3.5f) && near(right.point_volume[0], 4.75f));
        // above the ground far from the bodies; the same with a maximum distance below the gap is a miss
        auto up = world.distanceToSphere({20.f, 3.f, 0.f}, 0.5f);
        EXPECT(up.entity == ground.id && up.object_type == MI_OBJECT_STATIC_COLLIDER && near(up.distance, 2.5f) && near(up.normal[1], 1.f) && near(up.point_collider[1], 0.f) && near(up.point_volume[1], 2.5f));
        auto cut = world.distanceToSphere({20.f, 3.f, 0.f}, 0.5f, 2.4f);
        EXPECT(cut.entity == MI_RAY_MISS && cut.collider == MI_RAY_MISS && std::isinf(cut.distance) && cut.object_type == 0 && cut.flags == 0);
        EXPECT(world.distanceToSphere({20.f, 3.f, 0.f}, 0.5f, 2.6f).entity == ground.id);
        EXPECT(world.distanceToSphere({-2.f, 2.f, 0.f}, 0.25f, std::numeric_limits<float>::infinity(), MI_QUERY_STATIC).entity == ground.id);
        // inside the sphere body: an overlap (distance 0, both points the volume's pose position, no direction)
        auto inside = world.distanceToSphere({0.2f, 2.f, 0.f}, 0.25f);
        EXPECT(inside.entity == a.id && inside.distance == 0.f && (inside.flags & MI_DISTANCE_OVERLAP) && inside.normal[0] == 0.f && inside.point_collider[0] == 0.f && inside.point_volume[1] == 0.f);
        // batches, with and without maximum distances and entity ranges
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f; v.shape[0] = -2.f; v.shape[1] = 2.f; v.shape[3] = 0.25f;
        auto r = world.distance({v, v, v}, {10.f, 1.f, -1.f});
        EXPECT(r.size() == 3 && r[0].entity == a.id && r[1].entity == MI_RAY_MISS && r[2].entity == MI_RAY_MISS && r[2].volume == 2);
        auto ranged = world.distance({v, v}, {}, MI_QUERY_DEFAULT, {b.id, b.id + 1, 0u, 0xFFFFFFFFu});
        EXPECT(ranged[0].entity == b.id && near(ranged[0].distance, 4.5f - 0.25f) && ranged[1].entity == a.id);
        EXPECT(world.distance({}).empty());
        bool threw = false;
        try { world.distance({v}, {1.f, 2.f}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        std::printf("facade distance ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
