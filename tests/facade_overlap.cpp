// Runtime check of the overlap queries of include/physics_world.hpp (overlap with and without entity ranges, overlapSphere,
// overlapBox) against libmi_physics.so (run by tests/test_facade_overlap.py; executing it needs a GPU, compiling/linking does not).
#include <cstdio>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
int main() {
    try {
        physics_world world(0);
        physics_material mat{0.1f, 0.5f, 1.f};
        auto ground = world.addStaticCollider(trs{}, {collider_component::asAABB({-50, -4, -50}, {50, 0, 50}, mat)});
        trs t; t.position = {0, 2, 0};
        auto a = world.addRigidBody(t, rigid_body_component{}, {collider_component::asSphere({0, 0, 0}, 0.5f, mat)});
        t.position = {3, 2, 0};
        auto b = world.addRigidBody(t, rigid_body_component{}, {collider_component::asAABB({-0.5f, -0.5f, -0.5f}, {0.5f, 0.5f, 0.5f}, mat)});
        // single-volume conveniences (count, then fetch)
        auto s = world.overlapSphere({0.f, 2.f, 0.f}, 0.25f);
        EXPECT(s.size() == 1 && s[0].entity == a.id && s[0].object_type == MI_OBJECT_RIGID_BODY && s[0].volume == 0);
        EXPECT(world.overlapSphere({0.f, 10.f, 0.f}, 0.25f).empty());
        auto all = world.overlapSphere({1.5f, 1.f, 0.f}, 3.f);
        EXPECT(all.size() == 3 && all[0].collider < all[1].collider && all[1].collider < all[2].collider);
        EXPECT(world.overlapSphere({1.5f, 1.f, 0.f}, 3.f, MI_QUERY_STATIC).size() == 1);
        auto box = world.overlapBox({3.f, 2.f, 0.f}, {0.2f, 0.2f, 0.2f});
        EXPECT(box.size() == 1 && box[0].entity == b.id);
        const float h = 0.70710678f;
        auto turned = world.overlapBox({1.5f, 2.f, 0.f}, {1.2f, 0.1f, 0.1f}, quat{0.f, 0.f, h, h});       // its long axis turned onto y: touches neither body
        EXPECT(turned.empty());
        EXPECT(world.overlapBox({1.5f, 2.f, 0.f}, {1.2f, 0.1f, 0.1f}).size() == 2);
        // batches, with and without entity ranges
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f; v.shape[0] = 1.5f; v.shape[1] = 1.f; v.shape[3] = 3.f;
        mi_query_volume far = v; far.shape[1] = 40.f;
        auto r = world.overlap({v, far, v}, MI_QUERY_RIGID_BODIES | MI_QUERY_STATIC);
        EXPECT(r.offsets.size() == 4 && r.offsets[0] == 0 && r.offsets[1] == 3 && r.offsets[2] == 3 && r.offsets[3] == 6 && r.hits.size() == 6 && r.hits[5].volume == 2);
        auto ranged = world.overlap({v, far, v}, MI_QUERY_RIGID_BODIES | MI_QUERY_STATIC, {a.id, a.id + 1, 0u, 0xFFFFFFFFu, ground.id, ground.id + 1});
        EXPECT(ranged.hits.size() == 2 && ranged.hits[0].entity == a.id && ranged.hits[1].entity == ground.id && ranged.offsets[3] == 2);
        EXPECT(world.overlap({}).offsets.size() == 1);
        bool threw = false;
        try { world.overlap({v}, MI_QUERY_DEFAULT, {0u}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        std::printf("facade overlap ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
