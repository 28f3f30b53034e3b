// Runtime check of the shape-cast queries of include/physics_world.hpp (sweep with and without entity ranges, sweepSphere, sweepCapsule)
// against libmi_physics.so (run by tests/test_facade_sweep.py; executing it needs a GPU, compiling/linking does not).
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
        // a sphere of radius 0.25 from x = -4 along +x by 8: touches the sphere body when the centres are 0.75 apart: t = 3.25 / 8
        auto s = world.sweepSphere({-4.f, 2.f, 0.f}, 0.25f, {8.f, 0.f, 0.f});
        EXPECT(s.entity == a.id && s.object_type == MI_OBJECT_RIGID_BODY && s.flags == 0 && s.volume == 0);
        EXPECT(near(s.t, 3.25f / 8.f) && near(s.normal[0], -1.f) && near(s.normal[1], 0.f) && near(s.point[0], -0.5f) && near(s.point[1], 2.f));
        // from the other side the box comes first: its face x = 3.5 stops the centre at x = 3.75
        auto back = world.sweepSphere({8.f, 2.f, 0.f}, 0.25f, {-8.f, 0.f, 0.f});
        EXPECT(back.entity == b.id && near(back.t, 4.25f / 8.f) && near(back.normal[0], 1.f) && near(back.point[0], 3.5f));
        // downwards onto the ground; a cast that ends short of it is a miss
        auto down = world.sweepCapsule({10.f, 3.f, 0.f}, {10.f, 4.f, 0.f}, 0.5f, {0.f, -5.f, 0.f});
        EXPECT(down.entity == ground.id && down.object_type == MI_OBJECT_STATIC_COLLIDER && near(down.t, 0.5f) && near(down.normal[1], 1.f) && near(down.point[1], 0.f));
        auto shortCast = world.sweepCapsule({10.f, 3.f, 0.f}, {10.f, 4.f, 0.f}, 0.5f, {0.f, -2.f, 0.f});
        EXPECT(shortCast.entity == MI_RAY_MISS && shortCast.collider == MI_RAY_MISS && std::isinf(shortCast.t) && shortCast.object_type == 0);
        EXPECT(world.sweepSphere({-4.f, 2.f, 0.f}, 0.25f, {8.f, 0.f, 0.f}, MI_QUERY_STATIC).entity == MI_RAY_MISS);
        // starting inside the sphere body: an initial overlap (normal = -normalize(displacement))
        auto inside = world.sweepSphere({0.2f, 2.f, 0.f}, 0.25f, {1.f, 0.f, 0.f});
        EXPECT(inside.entity == a.id && inside.t == 0.f && (inside.flags & MI_SWEEP_INITIAL_OVERLAP) && near(inside.normal[0], -1.f) && inside.point[0] == 0.f);   // (point = the volume's pose position: sweepSphere leaves the pose at the origin)
        // batches, with and without entity ranges
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f; v.shape[0] = -4.f; v.shape[1] = 2.f; v.shape[3] = 0.25f;
        auto r = world.sweep({v, v, v}, {vec3{8.f, 0.f, 0.f}, vec3{0.f, 8.f, 0.f}, vec3{20.f, 0.f, 0.f}});
        EXPECT(r.size() == 3 && r[0].entity == a.id && r[1].entity == MI_RAY_MISS && r[2].entity == a.id && r[2].volume == 2 && near(r[2].t, 3.25f / 20.f));
        auto ranged = world.sweep({v, v}, {vec3{8.f, 0.f, 0.f}, vec3{8.f, 0.f, 0.f}}, MI_QUERY_DEFAULT, {b.id, b.id + 1, 0u, 0xFFFFFFFFu});
        EXPECT(ranged[0].entity == b.id && near(ranged[0].t, (2.5f - 0.25f + 4.f) / 8.f) && ranged[1].entity == a.id);
        EXPECT(world.sweep({}, {}).empty());
        bool threw = false;
        try { world.sweep({v}, {}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        std::printf("facade sweep ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
