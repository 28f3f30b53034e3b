// Runtime check of the contact-manifold query of include/physics_world.hpp (volumeContacts) against libmi_physics.so (run by
// tests/test_facade_volume_contacts.py; executing it needs a GPU, compiling/linking does not).  argv[1..8] = the expected bits of the
// single record's normal (3), point (3), depth and count_flags, as the oracle gives them for this pair (tests/contact_ref.py, sunk_sphere_case).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
    try {
        if (argc != 9) { std::printf("facade error: expected 8 words\n"); return 1; }
        uint32_t want[8];
        for (int i = 0; i < 8; ++i) want[i] = (uint32_t)std::strtoul(argv[1 + i], nullptr, 10);
        physics_world world(0);
        physics_material mat{0.1f, 0.5f, 1.f};
        auto box = world.addStaticCollider(trs{}, {collider_component::asAABB({-2, -1, -2}, {2, 0, 2}, mat)});
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f;
        v.shape[0] = 0.25f; v.shape[1] = 0.4f; v.shape[2] = -0.5f; v.shape[3] = 0.5f;     // sunk 0.1 into the box's top face
        mi_query_volume above = v; above.shape[1] = 0.6f;
        auto r = world.volumeContacts({above, v});
        EXPECT(r.offsets.size() == 3 && r.offsets[0] == 0 && r.offsets[1] == 0 && r.offsets[2] == 1 && r.contacts.size() == 1);
        const mi_volume_contact& c = r.contacts[0];
        EXPECT(c.entity == box.id && c.collider == 0 && c.object_type == MI_OBJECT_STATIC_COLLIDER && c.volume == 1);
        EXPECT(c.count_flags == 1u);                                  // one contact; the sphere (smaller type) was A: the normal points from it into the box
        EXPECT(c.normal[1] == -1.f && c.points[0][3] > 0.0999f && c.points[0][3] < 0.1001f);
        const uint32_t got[8] = {bits(c.normal[0]), bits(c.normal[1]), bits(c.normal[2]), bits(c.points[0][0]), bits(c.points[0][1]), bits(c.points[0][2]), bits(c.points[0][3]), c.count_flags};
        for (int i = 0; i < 8; ++i) if (got[i] != want[i]) { std::printf("facade error: word %d is %08x, the oracle's is %08x\n", i, got[i], want[i]); return 1; }
        for (int k = 1; k < 4; ++k) for (int j = 0; j < 4; ++j) EXPECT(bits(c.points[k][j]) == 0u);
        EXPECT(world.volumeContacts({}).offsets.size() == 1);
        EXPECT(world.volumeContacts({v}, MI_QUERY_RIGID_BODIES).contacts.empty());
        bool threw = false;
        try { world.volumeContacts({v}, MI_QUERY_DEFAULT, {0u}); } catch (const std::invalid_argument&) { threw = true; }
        EXPECT(threw);
        std::printf("facade volume contacts ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
