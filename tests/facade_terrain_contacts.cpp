// Runtime check of the terrain contact query of include/physics_world.hpp (terrainContacts) against libmi_physics.so (run by
// tests/test_facade_terrain_contacts.py; executing it needs a GPU, compiling/linking does not): a sphere sunk into flat terrain.
// argv[1..7] = the expected bits of the single record's point (3), depth and normal (3), as the oracle gives them for this case
// (tests/terrain_contact_ref.py, sunk_sphere_case).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "physics_world.hpp"
using namespace mi_facade;
#define EXPECT(c) do { if (!(c)) { std::printf("facade error: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
int main(int argc, char** argv) {
    try {
        if (argc != 8) { std::printf("facade error: expected 7 words\n"); return 1; }
        uint32_t want[7];
        for (int i = 0; i < 7; ++i) want[i] = (uint32_t)std::strtoul(argv[1 + i], nullptr, 10);
        physics_world world(0);
        mi_query_volume v{}; v.type = MI_COLLIDER_SPHERE; v.rotation[3] = 1.f;
        v.shape[0] = 3.3f; v.shape[1] = 2.4f; v.shape[2] = 4.7f; v.shape[3] = 0.5f;      // lowest point at y = 1.9
        EXPECT(world.terrainContacts({v}).contacts.empty());                              // no heightmap: nothing, and no error
        // one chunk of 16 m, every height 32768 of 65535, amplitude 4: a plane at y = 4 * 32768 / 65535 (just above 2)
        world.addHeightmap(1, 16.f, physics_material{0.05f, 0.8f, 1.f});
        std::vector<uint16_t> heights(129 * 129, (uint16_t)32768);
        world.setHeightmapChunk(0, 0, heights.data());
        world.updateHeightmap(vec3{0.f, 0.f, 0.f}, 4.f);
        mi_query_volume above = v; above.shape[1] = 2.6f;
        auto r = world.terrainContacts({above, v});
        // the sunk sphere's cap is narrower than a cell (12.4 cm): whatever its triangles give, the LAST record is the lowest-point contact
        EXPECT(r.offsets.size() == 3 && r.offsets[0] == 0 && r.offsets[1] == 0 && r.offsets[2] == r.contacts.size() && !r.contacts.empty());
        const mi_terrain_contact& c = r.contacts.back();
        EXPECT(c.volume == 1 && c.normal[0] == 0.f && c.normal[1] == -1.f && c.normal[2] == 0.f);
        EXPECT(c.depth > 0.1000f && c.depth < 0.1001f);                                   // 4 * 32768 / 65535 - 1.9 = 0.10003
        const uint32_t got[7] = {bits(c.point[0]), bits(c.point[1]), bits(c.point[2]), bits(c.depth), bits(c.normal[0]), bits(c.normal[1]), bits(c.normal[2])};
        for (int i = 0; i < 7; ++i) if (got[i] != want[i]) { std::printf("facade error: word %d is %08x, the oracle's is %08x\n", i, got[i], want[i]); return 1; }
        EXPECT(world.terrainContacts({}).offsets.size() == 1);
        std::printf("facade terrain contacts ok\n");
    } catch (const std::exception& e) {
        std::printf("facade error: %s\n", e.what());
        return 1;
    }
    return 0;
}
