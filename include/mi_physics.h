/*
 * mi_physics.h — C ABI of the MI355X-native rigid-body stepper.
 *
 * This is the drop-in boundary for the `src/physics` step path of pkurth/D3D12Renderer.
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repo root).  Plain pointers and sizes only; no C++ / torch types.  All functions
 * return MI_OK (0) or a negative mi_status; nothing throws across this boundary.
 *
 * Threading: one host thread per world.  All device work runs on a world-owned HIP stream;
 * every call returns after device completion.
 *
 * Index conventions (they matter for result parity):
 *   - rigid bodies are indexed in creation order (EnTT dense storage slot,
 *     src/physics/physics.cpp:654,1269-1273);
 *   - colliders are world-indexed in REVERSE creation order (EnTT iterates back to front,
 *     src/physics/physics.cpp:635-641);
 *   - a collider without a rigid body ("static collider") uses the dummy body index N_b
 *     (src/physics/physics.cpp:1214,1279).
 */
#ifndef MI_PHYSICS_H
#define MI_PHYSICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_API __attribute__((visibility("default")))

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_INVALID_ARGUMENT = -1,
    MI_ERR_NO_DEVICE = -2,        /* HIP device / kernels unavailable: the product path never falls back to CPU */
    MI_ERR_OUT_OF_MEMORY = -3,
    MI_ERR_DEVICE = -4,           /* a HIP call failed; see mi_last_error() */
    MI_ERR_CAPACITY = -5,
    MI_ERR_UNSUPPORTED = -6
} mi_status;

/* collider_type — src/physics/physics.h:59-70 (order is load-bearing: narrow-phase buckets). */
typedef enum mi_collider_type {
    MI_COLLIDER_SPHERE = 0,
    MI_COLLIDER_CAPSULE = 1,
    MI_COLLIDER_CYLINDER = 2,
    MI_COLLIDER_AABB = 3,
    MI_COLLIDER_OBB = 4,
    MI_COLLIDER_HULL = 5,
    MI_COLLIDER_TYPE_COUNT = 6
} mi_collider_type;

/* physics_object_type — src/physics/physics.h:49-57. */
typedef enum mi_object_type {
    MI_OBJECT_RIGID_BODY = 0,
    MI_OBJECT_STATIC_COLLIDER = 1,
    MI_OBJECT_FORCE_FIELD = 2,
    MI_OBJECT_TRIGGER = 3
} mi_object_type;

/* constraint_type — src/physics/constraints.h:14-28. */
typedef enum mi_constraint_type {
    MI_CONSTRAINT_DISTANCE = 0,
    MI_CONSTRAINT_BALL = 1,
    MI_CONSTRAINT_FIXED = 2,
    MI_CONSTRAINT_HINGE = 3,
    MI_CONSTRAINT_CONE_TWIST = 4,
    MI_CONSTRAINT_SLIDER = 5,
    MI_CONSTRAINT_TYPE_COUNT = 6
} mi_constraint_type;

enum { MI_ENTITY_DESTROYED = 0xFFFFFFFFu };   /* kind of an entity slot after mi_entity_destroy (read-back only) */
enum { MI_ENTITY_DYNAMIC = 0, MI_ENTITY_KINEMATIC = 1, MI_ENTITY_STATIC = 2,
       MI_ENTITY_TRIGGER = 3,        /* transform + trigger_component (src/physics/physics.h:200-203): colliders report enter / leave */
       MI_ENTITY_FORCE_FIELD = 4 };  /* transform + force_field_component (src/physics/physics.h:182-185): see mi_entity_set_force */

/*
 * An entity = transform_component (+ optional rigid_body_component).
 * Replaces: scene.createEntity().addComponent<transform_component>(pos, rot)
 *           .addComponent<rigid_body_component>(kinematic, gravityFactor, linearDamping, angularDamping)
 * (src/scene/scene.h:35-112, src/physics/rigid_body.cpp:6-27).  kind == MI_ENTITY_STATIC creates
 * the transform only: its colliders become static colliders.
 */
typedef struct mi_entity_desc {
    float position[3];
    float rotation[4];          /* quaternion x,y,z,w (src/core/math.h:292-298) */
    float linear_velocity[3];
    float angular_velocity[3];
    float gravity_factor;       /* default 1 */
    float linear_damping;       /* default 0.4 (src/physics/rigid_body.h:21) */
    float angular_damping;      /* default 0.4 */
    uint32_t kind;              /* MI_ENTITY_* */
} mi_entity_desc;

/*
 * collider_component::asSphere/asCapsule/asCylinder/asAABB/asOBB/asHull + physics_material
 * (src/physics/physics.h:108-171, 40-47).  Shapes are in the entity's local space.
 *   sphere   : shape = {cx,cy,cz, r}
 *   capsule  : shape = {ax,ay,az, bx,by,bz, r}
 *   cylinder : shape = {ax,ay,az, bx,by,bz, r}
 *   aabb     : shape = {minx,miny,minz, maxx,maxy,maxz}
 *   obb      : shape = {qx,qy,qz,qw, cx,cy,cz, rx,ry,rz}
 *   hull     : shape = {qx,qy,qz,qw, px,py,pz}, hull_geometry = id from mi_hull_geometry_create
 */
typedef struct mi_collider_desc {
    uint32_t type;              /* mi_collider_type */
    uint32_t object_type;       /* MI_OBJECT_RIGID_BODY (resolved from the entity) — force_field / trigger reserved */
    float shape[12];
    uint32_t hull_geometry;
    float restitution;
    float friction;
    float density;
} mi_collider_desc;

/* physics_settings minus callbacks — src/physics/physics.h:382-400. */
typedef struct mi_step_settings {
    uint32_t fixed_frame_rate;              /* bool, default 1 */
    uint32_t frame_rate;                    /* default 120 */
    uint32_t max_physics_iterations_per_frame; /* default 4 */
    uint32_t num_rigid_solver_iterations;   /* default 30 */
} mi_step_settings;

/* The bit-exact integers of one internal step (CPU_PROFILE_STAT names, src/physics/physics.cpp:1258-1262). */
typedef struct mi_step_counts {
    uint32_t num_rigid_bodies;
    uint32_t num_colliders;
    uint32_t num_broadphase_overlaps;
    uint32_t num_collisions;    /* manifolds */
    uint32_t num_contacts;
    uint32_t num_colors;        /* contact colours used by the solver schedule */
    uint32_t sorting_axis;      /* SAP axis used this step (src/physics/collision_broad.cpp:345) */
    uint32_t reserved;          /* product library: contact-solve kernel launches of the step */
} mi_step_counts;

/* collision_contact + constraint_body_pair + collider_pair — src/physics/physics.h:347-354. */
typedef struct mi_contact {
    float point[3];
    float penetration_depth;
    float normal[3];
    uint32_t friction_restitution;  /* 16:16 fixed point (src/physics/collision_narrow.cpp:2235-2238) */
    uint32_t collider_a, collider_b;
    uint32_t body_a, body_b;
} mi_contact;

/* Per-stage device time of the last internal step, milliseconds (profiler block names of SURVEY §5). */
typedef struct mi_stage_times {
    float world_colliders;
    float broadphase;
    float narrowphase;
    float integrate_forces;
    float schedule;
    float init_constraints;
    float solve;
    float integrate_velocities;
    float total;
} mi_stage_times;

typedef struct mi_world_desc {
    int32_t device;             /* HIP device ordinal */
    uint32_t flags;             /* reserved, 0 */
} mi_world_desc;

typedef struct mi_world mi_world;

/* Library */
MI_API const char* mi_last_error(void);
MI_API int mi_version(void);

/* physics_world ctor/dtor  <->  game_scene + memory_arena::initialize (src/physics/physics.cpp:1205). */
MI_API int mi_world_create(const mi_world_desc* desc, mi_world** out_world);
MI_API void mi_world_destroy(mi_world* world);

/* addRigidBody  <->  createEntity().addComponent<transform_component>()...addComponent<rigid_body_component>() */
MI_API int mi_entity_create(mi_world* world, const mi_entity_desc* desc, uint32_t* out_entity);
MI_API int mi_entities_create(mi_world* world, uint32_t count, const mi_entity_desc* descs, uint32_t* out_first_entity);
/*
 * game_scene::deleteEntity (src/scene/scene.cpp:124-150): the entity's colliders (removeColliderFromBroadphase,
 * src/physics/collision_broad.cpp:62-75), its constraints (deleteAllConstraintsFromEntity) and its rigid body / trigger / force field
 * go.  EnTT pool semantics decide the order everything else is processed in afterwards: in every component pool the LAST element
 * moves into the freed slot (rigid bodies, colliders — hence collider ids reported by events are pool positions and change for the
 * moved collider —, triggers, force fields).  Entity ids stay valid; the destroyed id is never reused.  The colour history and the
 * previous-step collision / trigger lists (which are keyed by pool positions) restart, so the next step reports every live
 * collision as begun again.
 */
MI_API int mi_entity_destroy(mi_world* world, uint32_t entity);
/* addComponent<collider_component>(collider_component::asXxx(shape, material)) (src/scene/scene.h:38-65). */
MI_API int mi_collider_add(mi_world* world, uint32_t entity, const mi_collider_desc* desc, uint32_t* out_collider);
MI_API int mi_colliders_add(mi_world* world, uint32_t count, const uint32_t* entities, const mi_collider_desc* descs);
/* allocateBoundingHullGeometry (src/physics/physics.cpp:58-84) / bounding_hull_geometry::fromMesh. */
MI_API int mi_hull_geometry_create(mi_world* world, const float* vertices_xyz, uint32_t num_vertices,
                                   const uint32_t* triangles_abc, uint32_t num_triangles, uint32_t* out_geometry);

/*
 * addConstraint(a, b, const xxx_constraint&) (src/physics/physics.h:235-240).  `pod` is laid out like the
 * reference structs (src/physics/constraints.h:73-80,129-135,175-183,229-257,346-380,497-520) with
 * 4-byte packing; see mi_*_constraint in mi_constraints.h.
 */
MI_API int mi_constraint_create(mi_world* world, uint32_t type, uint32_t entity_a, uint32_t entity_b,
                                const void* pod, uint32_t pod_bytes, uint32_t* out_constraint);
/* getConstraint(scene, handle) = mutable access (motors/limits) (src/physics/physics.h:244-249). */
MI_API int mi_constraint_update(mi_world* world, uint32_t type, uint32_t constraint, const void* pod, uint32_t pod_bytes);
MI_API int mi_constraint_get(mi_world* world, uint32_t type, uint32_t constraint, void* pod, uint32_t pod_bytes);
/* mi_constraint_update for `count` constraints of one type (pods = count consecutive PODs of pod_bytes each): a policy writing the
 * motor targets of thousands of ragdolls per step.  Updates only re-send the POD arrays; the step stays on its fast path. */
MI_API int mi_constraints_update(mi_world* world, uint32_t type, uint32_t count, const uint32_t* constraints, const void* pods, uint32_t pod_bytes);
/* deleteConstraint(scene, handle), deleteAllConstraints(scene), deleteAllConstraintsFromEntity(entity)
 * (src/physics/physics.h:251-260, physics.cpp:443-539).  Constraint ids stay valid across deletions of other constraints; the
 * solver's pool order follows EnTT's swap-and-pop (the last constraint of the type moves into the freed slot). */
MI_API int mi_constraint_destroy(mi_world* world, uint32_t type, uint32_t constraint);
MI_API int mi_constraints_destroy_all(mi_world* world);
MI_API int mi_entity_destroy_constraints(mi_world* world, uint32_t entity);
/* add{Distance,Ball,Fixed,Hinge,ConeTwist,Slider}ConstraintFromGlobalPoints (src/physics/physics.cpp:128-333). */
MI_API int mi_constraint_create_from_global(mi_world* world, uint32_t type, uint32_t entity_a, uint32_t entity_b,
                                            const float* global_anchor, const float* global_axis,
                                            float limit_min_or_swing, float limit_max_or_twist, uint32_t* out_constraint);

/* force_field_component::force (src/physics/physics.h:182-185) of a MI_ENTITY_FORCE_FIELD entity, in the entity's local frame
 * (getForceFieldStates rotates it by the transform, src/physics/physics.cpp:759-787).  With colliders the field is localized:
 * every overlap of one of its colliders with a rigid body's collider adds the force to that body for the step
 * (handleNonCollisionInteractions, physics.cpp:952-970); without colliders it is global and acts on every rigid body. */
MI_API int mi_entity_set_force(mi_world* world, uint32_t entity, const float* force3);

/*
 * Heightmap terrain — heightmap_collider_component (src/terrain/heightmap_collider.h:126-151), collided by heightmapCollision
 * (src/physics/heightmap_collision.cpp:509-618) right after the narrow phase, into the same contact arrays.  One per world.
 *   mi_heightmap_create            = heightmap_collider_component(chunksPerDim, chunkSize, material)
 *   mi_heightmap_set_chunk_heights = collider(x, z).setHeights(heights): 129 x 129 uint16, row-major [z][x]
 *                                    (TERRAIN_LOD_0_VERTICES_PER_DIMENSION); chunks without heights collide with nothing
 *   mi_heightmap_update            = update(minCorner, amplitudeScale): height = minCorner.y + h / 65535 * amplitudeScale
 *   mi_heightmap_get_height        = getHeightAt(coord): bilinear height, -FLT_MAX outside
 * Sphere, capsule, AABB and OBB colliders of rigid bodies collide with the terrain triangles (one contact per touched
 * triangle plus the lowest-point contact, at most 255 per collider); cylinders and hulls do not (the reference reads an
 * uninitialised point for them).  mi_contact::collider_b of a terrain contact is 0xFFFFFFFF and its body_b is the static dummy.
 * A stated deviation: the terrain stays at rest.  In the reference every terrain contact solves against one shared static body, and
 * an impulse that is not finite (a rigid body without mass: a sphere of radius 0, a box with a zero extent; its pose is NaN after its
 * first step wherever it is) enters that body's velocity as NaN x 0, so every body that touches the terrain in that step leaves it
 * with a NaN pose.  Here the static body's velocity is the constant 0: the NaN stays with the massless body and with what it touches
 * through collider contacts.  With finite numbers the two are the same bits.
 */
MI_API int mi_heightmap_create(mi_world* world, uint32_t chunks_per_dim, float chunk_size, float restitution, float friction);
MI_API int mi_heightmap_set_chunk_heights(mi_world* world, uint32_t chunk_x, uint32_t chunk_z, const uint16_t* heights129x129);
MI_API int mi_heightmap_update(mi_world* world, const float* min_corner3, float amplitude_scale);
MI_API int mi_heightmap_get_height(mi_world* world, float x, float z, float* out_height);

/* rb.forceAccumulator += f; rb.torqueAccumulator += tau (src/physics/physics.cpp:623-627). */
MI_API int mi_entity_apply_force(mi_world* world, uint32_t entity, const float* force3, const float* torque3);
/* The same for many rigid bodies at once, in order (either array may be NULL); added on the device when no topology edit is pending. */
MI_API int mi_entities_apply_forces(mi_world* world, uint32_t count, const uint32_t* entities, const float* forces3, const float* torques3);
/* testPhysicsInteraction(scene, ray, strength) (src/physics/physics.h:404, physics.cpp:555-629) for `count` rays, applied in
 * order: the closest rigid-body collider along ray i (ray::intersectSphere/Capsule/Cylinder/AABB/OBB/Hull in the entity's
 * physics_transform1 frame) receives force = direction * strength at the hit point.  strengths NULL = 1000 (the reference's
 * default); entity_ranges2 NULL = the whole scene, otherwise ray i only sees colliders of entities [lo_i, hi_i) — batched
 * environments in one world. */
MI_API int mi_world_test_interactions(mi_world* world, uint32_t count, const float* origins3, const float* directions3,
                                      const float* strengths, const uint32_t* entity_ranges2);

/*
 * Batched ray-cast scene queries: what does ray i hit first, where, and with what surface normal.  Read-only: the world's state and
 * every later step are unchanged.  The poses queried are physics_transform1 (those mi_world_test_interactions uses), pending host
 * edits included; the async variant sees the state at its point in the world's stream.
 *   - Per collider, t is what the reference's ray::intersect* returns in the entity's frame (the test mi_world_test_interactions
 *     runs), quirks included: a sphere that contains the origin reports t = 0 (a capsule too, unless its cylinder part answers first);
 *     a box (AABB / OBB) seen from inside reports no hit; the cylinder test (also the capsule's middle) can answer with a cap
 *     BEHIND the origin, and such a negative t is no hit (as any negative or non-finite t; mi_world_test_interactions still
 *     pushes a body whose only candidate is such a cap).  Seen from inside, a cylinder (and the middle of a capsule) finds that cap
 *     behind the origin, so no hit, for every direction with a part along the axis, and reports t = 0 for one exactly perpendicular
 *     to it; a hull seen from inside reports the triangle the ray LEAVES through: t > 0 and that triangle's outward normal, the one
 *     answer with dot(normal, direction) > 0 (the reference's triangle test does not cull back faces).
 *   - Direction length: only the boxes' slab test is independent of |direction|.  The reference's sphere test assumes a unit
 *     direction outright, its cylinder, cap-plane and triangle tests through absolute epsilons (1e-6 against b^2 - a c, against t and
 *     against dot(direction, normal)), so for spheres, capsules, cylinders and hulls the test runs on direction / |direction| and its t
 *     is rescaled: t is in the direction's units for every shape, and a ray hits the same point whatever its direction's length (tested
 *     from 1e-3 to 1e4).  A direction of length exactly 1 takes the reference's arithmetic unchanged.
 *   - Three deviations from the reference, each only where its test answers wrongly: a hull triangle whose edge cross product is shorter
 *     than 1e-4 (edges under about 1e-2), which the reference's noz() gives a zero normal and so never hits, is hit; an origin more than 32
 *     bounding radii in front of a sphere, capsule or cylinder is first moved along the ray to the shape's bounding sphere (the quadratics
 *     subtract r^2 from |origin - centre|^2 in float32: from 20 units a collider of 1e-2 was hit 5e-3 off, or missed); a cylinder the
 *     reference's test misses is tried once more with its comparisons of lengths widened from an absolute 1e-6 to a few float32 roundings of
 *     the coordinates (a ray aimed exactly at the rim passed between side and cap; the cap of a cylinder tens of units long was missed).
 *     A unit ray that starts within 32 radii and that the reference's test hits gets the reference's t, to the bit.
 *   - Limits that remain: t is good to about 5e-6 x the largest coordinate for round shapes (2e-5 from 6 units), 2e-7 x for boxes and
 *     hulls; a capsule or cylinder whose axis lies within 1e-3 rad of -y is placed about 1e-4 rad off (rotateFromTo next to its half turn);
 *     a cylinder's side of radius r stays invisible where r^2 - (distance from the axis)^2 < 1e-6.
 *   - The terrain: the heightmap's collision triangles (two per cell, as heightmap contacts use them; not the bilinear
 *     mi_heightmap_get_height surface, which they meet at the grid vertices and edges); chunks without heights are holes.  The
 *     surface is watertight: a ray whose segment crosses it is a hit wherever the origin lies, on a shared edge or vertex as anywhere
 *     else (the decision is a change of sign of the ray's height above the surface between points on the cells' rims that neighbouring
 *     cells compute alike, not an inclusion test of a rounded hit point per triangle).  It is hit from below as from above, with the
 *     triangle's upward normal; t is the crossing of the hit triangle's plane.  Accuracy: INTEGRATION.md, section 6b.
 *   - Closest hit = smallest t; ties go to the lowest world collider index; a collider wins a tie against the terrain.  A hit
 *     with t > max_t is a miss; so is a ray with a zero or non-finite direction or origin (never an error).  Cloth is not hit.
 *   - entity_ranges2 NULL = the whole scene, otherwise ray i sees the colliders of entities [lo_i, hi_i) only (the terrain, entity
 *     MI_RAY_TERRAIN, only when the range contains that value, i.e. the whole scene).
 *   - normal: unit, outward: sphere from the centre, capsule from the closest point of its segment, cylinder side or cap, box the
 *     entering slab's face, hull / terrain the hit triangle's normal; at t = 0 it is -normalize(direction).
 * A sharded world returns MI_ERR_UNSUPPORTED.  The accelerated structure (a uniform grid over the colliders' world AABBs) is built
 * on the device by the first query after anything moved, and reused until then.
 */
#define MI_RAY_MISS 0xFFFFFFFFu
#define MI_RAY_TERRAIN 0xFFFFFFFEu
typedef struct mi_ray_hit {
    uint32_t entity;      /* MI_RAY_MISS when nothing is hit; MI_RAY_TERRAIN for the heightmap */
    uint32_t collider;    /* world collider index, as in mi_contact; MI_RAY_MISS / MI_RAY_TERRAIN likewise */
    float t;              /* hit = origin + t * direction (direction need not be unit length); +inf on a miss */
    float point[3];       /* world space (0 on a miss) */
    float normal[3];      /* world space, unit, outward from the surface that was hit (0 on a miss) */
    uint32_t object_type; /* mi_object_type of the collider; MI_OBJECT_STATIC_COLLIDER for the terrain; 0 on a miss */
} mi_ray_hit;             /* 40 bytes */
enum {
    MI_QUERY_RIGID_BODIES = 1, MI_QUERY_STATIC = 2, MI_QUERY_TERRAIN = 4, MI_QUERY_TRIGGERS = 8, MI_QUERY_FORCE_FIELDS = 16,
    MI_QUERY_DEFAULT = 7
};
/* max_t NULL = +inf; include = MI_QUERY_* flags. */
MI_API int mi_world_raycast(mi_world* world, uint32_t count, const float* origins3, const float* directions3,
                            const float* max_t, uint32_t include, const uint32_t* entity_ranges2, mi_ray_hit* out);
/* Device buffers (e.g. torch tensors' data_ptr()), only enqueued on the world's stream (mi_world_get_stream): no host
 * synchronisation.  rays8_dev: per ray origin3, direction3, max_t, pad (16-byte aligned); ranges2_dev may be NULL. */
MI_API int mi_world_raycast_device_async(mi_world* world, uint32_t count, const float* rays8_dev, uint32_t include,
                                         const uint32_t* ranges2_dev, mi_ray_hit* out_dev);
/* The same result from the exhaustive scan over every collider and terrain cell (the yardstick of the accelerated path): byte for byte equal. */
MI_API int mi_debug_raycast_exhaustive(mi_world* world, uint32_t count, const float* origins3, const float* directions3,
                                       const float* max_t, uint32_t include, const uint32_t* entity_ranges2, mi_ray_hit* out);

/*
 * Batched volume-overlap queries: which colliders touch a shape right now.  Like the ray casts they read physics_transform1 (pending
 * host edits included), share the ray casts' grid (one build per pose epoch serves both) and change nothing a step computes.
 *   - A query volume is a collider in world space: type = mi_collider_type (sphere, capsule, cylinder, AABB, OBB, hull), shape laid
 *     out as mi_collider_desc::shape, hull_geometry an id of this world (hulls only), and a pose (position, rotation x,y,z,w) applied
 *     exactly as an entity's transform is applied to a static collider: an AABB under a rotation that is not exactly (0,0,0,1) becomes
 *     an OBB, as in the reference.  Use position 0 and rotation (0,0,0,1) for a shape given in world space.  The rotation is used as
 *     given, like an entity's: a quaternion that is not of unit length (the zero quaternion too) is not an error and not normalised.
 *   - World collider k is reported for volume v when (1) k's object type is selected by include (MI_QUERY_*), (2) k's entity lies in
 *     [lo_v, hi_v) when entity_ranges2 is given, (3) the world AABBs of v and k overlap as closed intervals (a collider whose AABB is
 *     not finite is never reported), and (4) the two shapes touch: they have a point in common.  What the query decides is the
 *     geometric answer for the float32 world shapes, up to a resolution per unit of scale = max(1, the largest |coordinate| of
 *     either shape).  MEASURED on the MI355X (tests/overlap_matrix.py: the 36 type pairs at sizes 5e-3 to 200 and coordinates up to
 *     1e3): every wrong answer was "overlapping" for shapes that are apart, by at most 4.7e-5 x scale; no overlapping pair was
 *     reported apart.  ASSERTED by the tests, the floor: the answer is right whenever the shapes are apart by, or have a common
 *     ball of radius, 8e-4 x scale (4 x the bound 2e-4 = 4 x the measured figure, one digit up); for the families that hold nothing
 *     finer (spheres and capsules about a cylinder's caps, contained shapes) 1.2e-3 x scale.  Closer to touching than the measured
 *     figure either answer may come.  The pairs of spheres and capsules among themselves, of a sphere with a box and of boxes among
 *     themselves are decided by the reference's closed forms of overlapCheck(A, B) (A = the smaller world type, sphere < capsule <
 *     cylinder < AABB < OBB < hull, a rotated AABB counts as OBB; the volume for equal types), bit for bit what a trigger computes;
 *     every other pair by the shape cast's distance search at a zero displacement, so mi_world_sweep's initial-overlap flag and this
 *     query agree on them.  A volume may be degenerate and decides as what it degenerates to: a sphere of radius 0 is a point, a
 *     capsule or cylinder of radius 0 a segment, a capsule of length 0 a sphere, a box with a zero extent a rectangle.  A cylinder of
 *     length 0 has no axis: what it reports is unspecified.
 *     What TRIGGERS in the step still do is the reference's overlapCheck on every pair, its quirks included, and the query no longer
 *     mirrors them: (a) sphere or capsule against a cylinder beyond its caps: a squared distance is compared with a radius, so a
 *     small sphere beside a rim enters a trigger it is clear of, and a large one deep in a cap does not; (b) every pair with a
 *     cylinder or a hull, and a capsule against a box, are GJK with absolute thresholds (|direction|^2 < 1e-4, +-1e-5), its error
 *     paths reading as "no overlap": shapes of a few centimetres enter nothing, and grazing overlaps of some millimetres are missed
 *     at any size; (c) a capsule of length 0 divides by its length.
 *   - Not reported: the terrain (the reference has no boolean test against the heightmap; MI_QUERY_TERRAIN is accepted and ignored;
 *     mi_world_terrain_contacts below reports where a volume touches the terrain, and its count-only call whether it does) and cloth.
 *     A sharded world returns MI_ERR_UNSUPPORTED.
 *   - An invalid volume (a non-finite number among the words its type reads or in its pose, a type out of range, an unknown hull
 *     geometry, a negative radius or half-extent, an AABB with max < min, a world AABB that overflows) reports nothing: an empty
 *     segment, never an error.
 *   - Result (CSR): out_offsets[count + 1], and the records of volume v at [out_offsets[v], out_offsets[v + 1]) in ascending world
 *     collider index, each collider once.  The order is part of the contract.
 *   - Capacity: out_total always receives the full number of records and out_offsets the full offsets.  When that number exceeds
 *     capacity, the first `capacity` records (in result order) are written and MI_ERR_CAPACITY is returned; out_hits NULL with
 *     capacity 0 is the count-only call and returns MI_OK.
 */
typedef struct mi_query_volume {   /* 96 bytes, 16-byte aligned rows: usable from the host and as a device buffer */
    uint32_t type; uint32_t hull_geometry; float shape[12];
    float position[3]; float pad0; float rotation[4]; float pad1[2];
} mi_query_volume;
typedef struct mi_overlap_hit { uint32_t entity, collider, object_type, volume; } mi_overlap_hit;   /* 16 bytes */
MI_API int mi_world_overlap(mi_world* world, uint32_t count, const mi_query_volume* volumes, uint32_t include,
                            const uint32_t* entity_ranges2, uint32_t* out_offsets, mi_overlap_hit* out_hits, uint32_t capacity,
                            uint32_t* out_total);
/* Device buffers (16-byte aligned), only enqueued on the world's stream: no host synchronisation.  The same truncation rule:
 * total_dev[0] receives the full count (so the consumer can detect truncation), offsets_dev the full offsets, and nothing is
 * written at or past hits_dev[capacity].  ranges2_dev may be NULL; hits_dev may be NULL when capacity is 0. */
MI_API int mi_world_overlap_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev, uint32_t include,
                                         const uint32_t* ranges2_dev, uint32_t* offsets_dev, mi_overlap_hit* hits_dev,
                                         uint32_t capacity, uint32_t* total_dev);
/* The same result from every collider tested against every volume, without the grid and from collider rows computed for the
 * call (the yardstick of the accelerated path): byte for byte equal. */
MI_API int mi_debug_overlap_exhaustive(mi_world* world, uint32_t count, const mi_query_volume* volumes, uint32_t include,
                                       const uint32_t* entity_ranges2, uint32_t* out_offsets, mi_overlap_hit* out_hits,
                                       uint32_t capacity, uint32_t* out_total);

/*
 * Batched shape casts (sweeps): move a volume along a displacement and report the first collider it touches, where, and with what normal
 * (a character controller's move, a foot or ground probe, a projectile with thickness, a spawn check).  The volumes, their validation (an
 * invalid one is a miss, never an error), their pose handling (an AABB under a rotation that is not exactly (0,0,0,1) is an OBB), the
 * include flags, entity_ranges2 and the pose read (physics_transform1, pending edits included) are those of mi_world_overlap; the casts share
 * the grid of the other queries and change nothing a step computes.  A sharded world returns MI_ERR_UNSUPPORTED.
 *   - The motion: volume i keeps its orientation and moves from its pose by t * displacement_i, t in [0, 1].  The hit is the smallest t at
 *     which volume and collider touch; ties go to the lowest world collider index.  Closest hit only; translation only.  A zero
 *     displacement is valid (it reports an initial overlap or a miss); a non-finite displacement is a miss.
 *   - A hit: normal is a unit separating direction at the moment of touch, pointing from the collider to the volume (moving the volume
 *     along it leaves the collider), dot(normal, displacement) <= 0; point lies on the collider's surface; t is a fraction of the
 *     displacement.  Spheres and capsules are swept as a point / segment with a radius, so their normals are exact and a sphere of radius
 *     0 is a ray.
 *   - Initial overlap (the volume touches a collider at its pose): t = 0, MI_SWEEP_INITIAL_OVERLAP is set, normal =
 *     -normalize(displacement) (0 for a zero displacement), point = the volume's pose position.  For penetration data call
 *     mi_world_volume_contacts.
 *   - Termination: the pair test (a GJK-based convex cast) runs at most 32 iterations.  Its t only advances by clips that cannot pass the
 *     true time of impact, so a pair that reaches the limit, or whose search stalls more than 16 distance tolerances (2e-6 x the largest
 *     coordinate each) from the touch, reports its current t, a lower bound, with MI_SWEEP_UNCONVERGED: conservative, never a silent miss.
 *     In practice (all 36 volume type x collider type pairs at parallel faces, edges and axes, grazing passes, coordinates up to 1e3,
 *     sizes from 1e-2 to 200, displacements from 1e-3 to 1e4, starts and ends a hair from the touch): the flag appeared only for a box of
 *     1e-2 on the curved side of a cylinder of radius 15, with t 1e-4 x the coordinates early and the hit itself right.
 *   - Accuracy (float32, measured against a float64 reference; "coordinates" = the largest |coordinate| of the cast, at least 1): t times
 *     the displacement's length is within 5e-6 x coordinates of the true travelled distance (1.1e-4 x in the unconverged case above) and
 *     passes it by no more than 2e-7 x coordinates; point lies within 1e-7 x coordinates of the collider's surface.
 *   - The terrain (MI_QUERY_TERRAIN) is what the ray cast hits: the heightmap's collision triangles, two per cell, (A, B, C) and
 *     (C, B, D).  They are two-sided surfaces with no volume below them; chunks without heights are holes; outside the map there is
 *     nothing.  It is tested when the world has a heightmap, include has MI_QUERY_TERRAIN and the cast's entity range contains
 *     MI_RAY_TERRAIN (a NULL range means the whole scene): the ray cast's rule.  In every other case the call does what it does without
 *     the bit.  A terrain hit has entity = collider = MI_RAY_TERRAIN and object_type = MI_OBJECT_STATIC_COLLIDER; t is the fraction of
 *     the displacement, point lies on the triangle, normal is unit, points from the terrain towards the volume and has
 *     dot(normal, displacement) <= 0: a volume that comes from below gets a normal that points down.  Spheres and capsules keep their
 *     point / segment-plus-radius treatment; on flat ground the normal of a round volume of radius r is within 2 sqrt(tolerance / r) of
 *     the surface's (the distance tolerance above; the touch may be found on a neighbouring triangle that far beside the foot point).
 *     A volume without a radius (a box, a hull, a cylinder's flat end, a sphere of radius 0) that meets an edge or a vertex of the terrain
 *     reports the last clip plane's normal: a separating direction of the volume and the triangle hit (moving the volume along it leaves
 *     the terrain), not the normal of a neighbouring face; for a sphere of radius 0 it lies between the reversed direction of travel and
 *     the faces' normals (measured: up to 25 degrees off them), where mi_world_raycast reports the face's normal.
 *     A collider wins a tie in t against the terrain, as in the ray cast; among triangles the lowest (gz * n + gx) * 2 + tri wins
 *     (n = chunks per dimension x 128), so both kernels give the same point and normal.  Initial overlap (the volume touches a triangle at
 *     its pose) is reported as for colliders.  A volume wholly below the surface touches no triangle: it is cast from where it is and
 *     can hit the surface from below; for penetration against the terrain call mi_world_terrain_contacts.  Accuracy on the terrain, as
 *     above and per unit of coordinates: see INTEGRATION.md, section 6f.  The terrain is tested in a launch of its own behind the
 *     colliders': a terrain hit does not shorten the collider pass.  Heightmaps of more than 256 chunks per dimension return
 *     MI_ERR_UNSUPPORTED when the terrain is asked for.
 *   - Not hit: cloth.  Also out of scope: rotation during the sweep, all-hits and any-hit variants, and the terrain in mi_world_overlap
 *     and mi_world_volume_contacts.  The distance of a volume from the terrain (ground clearance) comes from mi_world_terrain_distance.
 *   - Result: one record per cast, out[count].
 */
typedef struct mi_sweep_hit {   /* 48 bytes, 16-byte aligned rows: usable from the host and as a device buffer */
    uint32_t entity, collider;  /* MI_RAY_MISS when nothing is hit; collider = world collider index; both MI_RAY_TERRAIN for the heightmap */
    float t;                    /* fraction of the displacement in [0,1]; +inf on a miss */
    uint32_t object_type;       /* mi_object_type of the collider (MI_OBJECT_STATIC_COLLIDER for the terrain); 0 on a miss */
    float point[3];             /* world space, on the collider's surface or the terrain triangle (0 on a miss) */
    uint32_t flags;             /* MI_SWEEP_* */
    float normal[3];            /* world space, unit, from the collider or the terrain towards the volume (0 on a miss) */
    uint32_t volume;            /* index of the cast */
} mi_sweep_hit;
enum { MI_SWEEP_INITIAL_OVERLAP = 1, MI_SWEEP_UNCONVERGED = 2 };
/* displacements3: three floats per cast. */
MI_API int mi_world_sweep(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* displacements3,
                          uint32_t include, const uint32_t* entity_ranges2, mi_sweep_hit* out);
/* Device buffers (16-byte aligned), only enqueued on the world's stream: no reservation and no host synchronisation.
 * displacements4_dev: one row of 16 bytes per cast (x, y, z; w is ignored); ranges2_dev may be NULL. */
MI_API int mi_world_sweep_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev, const float* displacements4_dev,
                                       uint32_t include, const uint32_t* ranges2_dev, mi_sweep_hit* out_dev);
/* The same result from every collider tested against every cast, without the grid, without skipping by the best time so far and from
 * collider rows computed for the call, and from every terrain triangle without the height mips (the yardstick of the accelerated path):
 * byte for byte equal. */
MI_API int mi_debug_sweep_exhaustive(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* displacements3,
                                     uint32_t include, const uint32_t* entity_ranges2, mi_sweep_hit* out);

/*
 * Batched distance queries: how far is a shape from the nearest collider, and which two points realise that distance (what PhysX calls
 * computeDistance and Bullet closest points: proximity sensors, clearance checks, placement, steering, observations).  The volumes, their
 * validation (an invalid one is a miss, never an error), their pose handling, the include flags, entity_ranges2, the pose read
 * (physics_transform1, pending edits included) and the pose epoch are those of mi_world_sweep; the queries share the grid of the other
 * queries and change nothing a step computes.  A sharded world returns MI_ERR_UNSUPPORTED.
 *   - Reported for volume v: the admitted collider (object type selected by include, entity in [lo_v, hi_v), a finite world AABB) with the
 *     smallest distance, if that distance is <= max_distance_v; ties go to the lowest world collider index.  max_distances NULL = +inf for
 *     every volume; +inf is allowed; a negative or NaN max_distance is a miss.  A world without colliders reports misses.
 *   - distance is the distance between the two float32 world shapes; point_collider lies on the collider's surface, point_volume on the
 *     volume's; normal = normalize(point_volume - point_collider), unit, from the collider towards the volume.  Spheres and capsules are a
 *     point or segment core plus a radius, as in the casts, so their figures are exact up to rounding.  Where the closest points are not
 *     unique (parallel faces, edges, a cap flat on a face) any pair that realises the distance may be reported.
 *   - Shapes that touch or overlap: distance = 0, MI_DISTANCE_OVERLAP is set, both points are the volume's pose position and normal is 0.
 *     For penetration data call mi_world_volume_contacts.  Among several overlapping colliders the lowest index wins (the tie rule).  The
 *     decision is the shape cast's for an initial overlap: no support plane separates the shapes by more than the search's tolerance.
 *   - Termination: the pair test (GJK on the cores' Minkowski difference) runs at most 64 iterations and stops by a tolerance relative to the
 *     coordinates (2e-6 x the largest coordinate, no absolute threshold).  Its running distance is an upper bound of the true one, so a
 *     pair that reaches the limit, or whose search stalls more than 16 tolerances from its lower bound, reports its current distance with
 *     MI_DISTANCE_UNCONVERGED: too far, never too near.
 *   - The reported distance is never below the gap of the two world AABBs (the bound candidates are skipped by): it is the pair test's
 *     distance raised to that gap, which differs from it by roundings only.
 *   - Accuracy (float32, measured against a float64 reference): see INTEGRATION.md, section 6g.
 *   - Not reported: the terrain (the MI_QUERY_TERRAIN bit changes nothing here; the distance to the heightmap comes from
 *     mi_world_terrain_distance, below, which can merge into these records) and cloth.  Also out of scope: k-nearest and all-within
 *     variants.
 *   - Result: one record per volume, out[count].
 */
typedef struct mi_distance_hit {   /* 64 bytes, four 16-byte rows: usable from the host and as a device buffer */
    uint32_t entity, collider;     /* MI_RAY_MISS when nothing lies within max_distance; collider = world collider index */
    float distance;                /* >= 0; +inf on a miss */
    uint32_t object_type;          /* mi_object_type of the collider; 0 on a miss */
    float point_collider[3];       /* world space, on the collider's surface (0 on a miss) */
    uint32_t flags;                /* MI_DISTANCE_* */
    float point_volume[3];         /* world space, on the volume's surface (0 on a miss) */
    uint32_t volume;               /* index of the query */
    float normal[3];               /* world space, unit, from the collider towards the volume (0 on a miss or an overlap) */
    uint32_t pad;
} mi_distance_hit;
enum { MI_DISTANCE_OVERLAP = 1, MI_DISTANCE_UNCONVERGED = 2 };
/* max_distances: one float per volume, or NULL (+inf). */
MI_API int mi_world_distance(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* max_distances,
                             uint32_t include, const uint32_t* entity_ranges2, mi_distance_hit* out);
/* Device buffers (16-byte aligned records and volumes), only enqueued on the world's stream: no reservation and no host synchronisation.
 * max_distances_dev (one float per volume) and ranges2_dev may be NULL. */
MI_API int mi_world_distance_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev, const float* max_distances_dev,
                                          uint32_t include, const uint32_t* ranges2_dev, mi_distance_hit* out_dev);
/* The same result from every collider tested against every volume, without the grid, without skipping by the best distance so far and from
 * collider rows computed for the call (the yardstick of the accelerated path): byte for byte equal. */
MI_API int mi_debug_distance_exhaustive(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* max_distances,
                                        uint32_t include, const uint32_t* entity_ranges2, mi_distance_hit* out);

/*
 * Batched terrain distance queries: how far is a shape from the heightmap terrain, and which two points realise that distance (ground
 * clearance of a foot capsule, a wheel hull or a chassis box over rolling ground; the nearest terrain point for steering and placement).
 * The terrain's own entry point beside mi_world_distance, as mi_world_terrain_contacts stands beside mi_world_volume_contacts; the
 * volumes, their validation (mi_world_overlap's) and their pose handling are those of mi_world_distance, the record is mi_distance_hit.
 * There are no include flags and no entity ranges.  Read-only for the step.  A sharded world returns MI_ERR_UNSUPPORTED.
 *   - The terrain is what the ray cast and the shape cast hit: the heightmap's collision triangles, two per cell, (A, B, C) and
 *     (C, B, D): two-sided surfaces with no volume below them; chunks without heights are holes.  A volume wholly below the surface has a
 *     positive distance and a normal that points down.  Unlike a cast, a volume beside the map still has a nearest triangle, on the rim:
 *     this is a distance, not an intersection.
 *   - Reported for volume v: the triangle with the smallest distance, if that distance is <= max_distance_v, as entity = collider =
 *     MI_RAY_TERRAIN and object_type = MI_OBJECT_STATIC_COLLIDER; otherwise a miss of mi_world_distance's shape.  max_distances NULL =
 *     +inf for every volume; a negative or NaN max_distance is a miss.  point_collider lies on the triangle, point_volume on the volume,
 *     normal = normalize(point_volume - point_collider).  Spheres and capsules stay a point or segment core plus a radius.  Among
 *     triangles at equal distance the lowest (gz * n + gx) * 2 + tri wins (cell (gx, gz) of the whole map, n = chunks per dimension x
 *     128), the casts' rule; which of two neighbours that share the closest edge or vertex is meant is not observable in the record.
 *   - A volume that touches a triangle: distance = 0, MI_DISTANCE_OVERLAP, both points the pose position, normal 0.  The decision is the
 *     shape cast's for an initial overlap.  MI_DISTANCE_UNCONVERGED means what it means for colliders: too far, never too near.
 *   - The reported distance is the pair test's raised to the gap of the volume's AABB and the triangle's (roundings only): the bound by
 *     which cells, 8 x 8 blocks and chunks are skipped through the height mips, strictly, so the accelerated walk and the exhaustive
 *     yardstick agree byte for byte.
 *   - An invalid volume is a miss when merge == 0 and is left untouched when merge != 0.
 *   - merge != 0: out holds the records of a mi_world_distance call for the same volumes (the blocking call reads and writes out).  A
 *     record is replaced only when it is a miss or the terrain is strictly nearer: a collider wins a tie, as in the casts.  The
 *     existing distance also bounds the search.  Every record that is not replaced keeps its bytes.  Two enqueues thus give "the
 *     nearest of anything" without host work.
 *   - A world without a heightmap returns MI_OK: misses when merge == 0, nothing written when merge != 0.  A heightmap of more than 256
 *     chunks per dimension returns MI_ERR_UNSUPPORTED (the casts' limit).
 *   - The heightmap buffers are read as the casts read them: mi_heightmap_set_chunk_heights and mi_heightmap_update are followed by
 *     the next query.
 *   - Accuracy (float32, measured against a float64 reference): see INTEGRATION.md, section 6h.
 *   - Result: one record per volume, out[count].
 */
MI_API int mi_world_terrain_distance(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* max_distances,
                                     uint32_t merge, mi_distance_hit* out);
/* Device buffers (16-byte aligned records and volumes), only enqueued on the world's stream: no reservation and no host synchronisation.
 * max_distances_dev (one float per volume) may be NULL.  With merge != 0 out_dev is read and written: enqueue it behind
 * mi_world_distance_device_async on the same buffers. */
MI_API int mi_world_terrain_distance_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev,
                                                  const float* max_distances_dev, uint32_t merge, mi_distance_hit* out_dev);
/* The same result from every triangle of every chunk that has heights, without the height mips and without skipping by the best distance
 * so far (the yardstick of the accelerated path): byte for byte equal. */
MI_API int mi_debug_terrain_distance_exhaustive(mi_world* world, uint32_t count, const mi_query_volume* volumes, const float* max_distances,
                                                uint32_t merge, mi_distance_hit* out);

/*
 * Batched contact-manifold queries: where a shape touches the world, along which normal and how deep (what PhysX calls
 * computePenetration and Bullet contactTest).  The volumes, their validation (an invalid one yields an empty segment), the include
 * flags, entity_ranges2, the pose read (physics_transform1, pending edits included), the CSR result in ascending world collider index
 * and the capacity protocol are those of mi_world_overlap; a sharded world returns MI_ERR_UNSUPPORTED.
 *   - World collider k is reported for volume v when it passes (1) the object-type filter, (2) the entity-range test and (3) the closed
 *     world-AABB test of mi_world_overlap, and the step's narrow phase, run on (A, B), returns at least one contact.  A is the one of
 *     the two with the smaller world type (sphere < capsule < cylinder < AABB < OBB < hull); for equal types A is the volume.
 *   - A record holds the narrow phase's own bits for that (A, B): the manifold a rigid body of the volume's shape at the volume's pose
 *     would get from one step against that collider as (A, B).  Nothing is negated or re-ordered; bit 8 of count_flags says which of
 *     the two the volume was.
 *   - The normal is a unit vector pointing from A to B, as the reference's (sphereSphere: normalize(centre B - centre A)); points[i] =
 *     (world contact point, penetration depth >= 0).  To separate the volume from the collider move the VOLUME along -normal when it
 *     was A (bit 8 clear) and along +normal when it was B (bit 8 set), by the largest depth of the record.
 *   - Not reported: the terrain (MI_QUERY_TERRAIN is accepted and ignored, as by mi_world_overlap; a volume's terrain contacts come from
 *     mi_world_terrain_contacts below) and cloth.
 */
typedef struct mi_volume_contact {   /* 96 bytes, 16-byte aligned rows: usable from the host and as a device buffer */
    uint32_t entity, collider, object_type, volume;   /* as mi_overlap_hit */
    float normal[3]; uint32_t count_flags;            /* bits 0..2: contacts (1..4); bit 8: the volume was B of the pair */
    float points[4][4];                               /* world point xyz + penetration depth; unused rows are 0 */
} mi_volume_contact;
MI_API int mi_world_volume_contacts(mi_world* world, uint32_t count, const mi_query_volume* volumes, uint32_t include,
                                    const uint32_t* entity_ranges2, uint32_t* out_offsets, mi_volume_contact* out_contacts,
                                    uint32_t capacity, uint32_t* out_total);
/* Sizes the library's candidate staging (about 150 bytes per candidate; a candidate = a collider that passes tests (1)-(3)).  The
 * host call grows it by itself; the device call uses what was reserved.  Grow-only; synchronises the world's stream. */
MI_API int mi_world_volume_contacts_reserve(mi_world* world, uint32_t max_candidates);
/* Device buffers (16-byte aligned), only enqueued on the world's stream: no host synchronisation.  totals2_dev[0] receives the
 * records, totals2_dev[1] the candidates found.  When the candidates exceed the reservation, only the first reserved candidates (in
 * result order) are evaluated: totals2_dev[1] > the reservation tells the consumer that records, offsets and totals2_dev[0] are those
 * of that prefix.  Nothing is written at or past contacts_dev[capacity].  With nothing reserved the call returns MI_ERR_CAPACITY. */
MI_API int mi_world_volume_contacts_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev, uint32_t include,
                                                 const uint32_t* ranges2_dev, uint32_t* offsets_dev, mi_volume_contact* contacts_dev,
                                                 uint32_t capacity, uint32_t* totals2_dev);
/* Device times of the narrow phase of the last contact query made while mi_world_set_stage_timing was on (0 otherwise), milliseconds:
 * out_ms3 = { the primitive / box kernel, the GJK kernel, all of narrow phase + compaction }.  The candidate passes before them are not
 * included.  Synchronises with that query. */
MI_API int mi_debug_volume_contacts_times(mi_world* world, float* out_ms3);
/* The same result with the candidates taken from every collider against every volume, without the grid and from collider rows
 * computed for the call: byte for byte equal. */
MI_API int mi_debug_volume_contacts_exhaustive(mi_world* world, uint32_t count, const mi_query_volume* volumes, uint32_t include,
                                               const uint32_t* entity_ranges2, uint32_t* out_offsets, mi_volume_contact* out_contacts,
                                               uint32_t capacity, uint32_t* out_total);

/*
 * Batched terrain contact queries: where a shape touches the heightmap terrain (the ground under a character's capsule, a foot probe,
 * a spawn test).  The volumes, their validation (an invalid one yields an empty segment) and their pose handling (an AABB under a
 * rotation that is not exactly (0,0,0,1) is an OBB) are those of mi_world_overlap; like every query it reads the current scene
 * (pending host edits, heightmap edits included, are uploaded first) and changes nothing a step computes.  A sharded world returns
 * MI_ERR_UNSUPPORTED.  There are no include flags and no entity ranges: the terrain is one object.
 *   - Volume v reports exactly the contacts a rigid body of that shape at that pose would get from the terrain in one step
 *     (the reference's heightmapCollision), with the same bits in point, depth and normal, in the reference's emission order: the
 *     triangle contacts in the order of its walk down the min/max quadtree (a stack: descending Morton code of the cell with x as the
 *     high bit, a cell's first triangle before its second; chunk rows z ascending, x ascending within a row), then the lowest-point
 *     contact.  At most 255 contacts per volume (the reference's limit); what would follow is dropped.
 *   - Per shape: spheres, capsules, AABBs and OBBs test the triangles of their cell window and add the lowest-point contact; cylinders
 *     and hulls get the lowest-point contact only, as in the step.  The lowest-point contact: the volume's support point along
 *     (0,-1,0) lies under the bilinear surface; point = that support point, depth = surface height - point.y, normal = (0,-1,0).
 *   - The normal is a unit vector from the volume towards the terrain: move the volume along -normal by depth to separate it.
 *   - Holes and map edges: a chunk without heights is a hole and reports nothing; a world without a heightmap reports nothing (all
 *     offsets 0) and returns MI_OK.  The cell window of a volume, the extension of its world AABB by 10 upwards before the window and
 *     the height range are taken, and the clamping of the window at the map's edge are the step's own (one code runs both).
 *   - Result (CSR): out_offsets[count + 1], and the records of volume v at [out_offsets[v], out_offsets[v + 1]) in emission order.
 *     The order is part of the contract.
 *   - Capacity: exactly the protocol of mi_world_overlap.  out_total always receives the full number of records and out_offsets the
 *     full offsets; the first `capacity` records in result order are written (a cut may fall inside a volume's segment), nothing at
 *     or past out_contacts[capacity]; a truncated result returns MI_ERR_CAPACITY; out_contacts NULL with capacity 0 is the count-only
 *     call and returns MI_OK.
 */
typedef struct mi_terrain_contact {   /* 32 bytes, 16-byte aligned rows: usable from the host and as a device buffer */
    float point[3]; float depth;      /* world contact point, penetration depth */
    float normal[3]; uint32_t volume; /* unit, from the volume towards the terrain (lowest-point contact: (0,-1,0)); index of the volume */
} mi_terrain_contact;
MI_API int mi_world_terrain_contacts(mi_world* world, uint32_t count, const mi_query_volume* volumes, uint32_t* out_offsets,
                                     mi_terrain_contact* out_contacts, uint32_t capacity, uint32_t* out_total);
/* Device buffers (16-byte aligned), only enqueued on the world's stream: no host synchronisation, and no reservation (the staging
 * per volume is sized from count by the call).  total_dev[0] receives the full count, offsets_dev the full offsets, and nothing is
 * written at or past contacts_dev[capacity]; contacts_dev may be NULL when capacity is 0. */
MI_API int mi_world_terrain_contacts_device_async(mi_world* world, uint32_t count, const mi_query_volume* volumes_dev,
                                                  uint32_t* offsets_dev, mi_terrain_contact* contacts_dev, uint32_t capacity,
                                                  uint32_t* total_dev);

/* physicsStep(scene, arena, timer, settings, dt) (src/physics/physics.cpp:1364-1413). */
MI_API int mi_world_step(mi_world* world, const mi_step_settings* settings, float dt);
/* n × physicsStepInternal(scene, arena, settings, dt) (src/physics/physics.cpp:1180-1362); no interpolation. */
MI_API int mi_world_step_fixed(mi_world* world, const mi_step_settings* settings, float dt, uint32_t num_steps);

/* One internal step with a HIP event pair around every contact-solver launch (the dominant kernel: k_contact_solve_flow,
 * or k_contact_solve per colour with MI_SOLVER=launch): returns the number of launches, their summed device time and the
 * contact updates (contacts x iterations) they performed. */
MI_API int mi_world_step_profiled(mi_world* world, const mi_step_settings* settings, float dt, uint32_t* out_launches,
                                  float* out_kernel_ms, uint64_t* out_contact_updates);

/* Stepping statistics since world creation: internal steps taken, steps run speculatively (one host read-back at the end,
 * sizes bounded from the previous step) and how many of those had to be re-run synchronously because a bound was exceeded. */
MI_API int mi_world_get_step_mode_stats(mi_world* world, uint32_t* out_steps, uint32_t* out_speculative, uint32_t* out_retries);

/* Read-back (transform_component / rigid_body_component fields), entity order. */
MI_API int mi_world_num_entities(mi_world* world, uint32_t* out);
MI_API int mi_world_get_transforms(mi_world* world, float* positions_xyz, float* rotations_xyzw, uint32_t capacity);
MI_API int mi_world_get_physics_transforms(mi_world* world, float* positions_xyz, float* rotations_xyzw, uint32_t capacity);
/* The same values without the last host copy, for a caller that reads every entity's transform after every step (the renderer
 * reading transform_component, src/physics/physics.cpp:1392-1411): pointers to the library's pinned host rows, [count][3] positions
 * and [count][4] rotations.  The rows are produced on the device in this layout and cross the bus as ONE copy which, once a caller
 * has asked after a step, every later step enqueues itself before it returns.  Valid until the SECOND next stepping call on this
 * world (two sets alternate) or until entities are added; read-only.  MI_ERR_UNSUPPORTED when the poses are not coming from the device right now (nothing
 * stepped since the last full download, a topology change is pending, a sharded world): mi_world_get_transforms covers every case. */
MI_API int mi_world_view_transforms(mi_world* world, const float** positions_xyz, const float** rotations_xyzw, uint32_t* out_count);
MI_API int mi_world_view_physics_transforms(mi_world* world, const float** positions_xyz, const float** rotations_xyzw, uint32_t* out_count);
/* The same rows WITHOUT waiting for a copy that is still on the bus: the NEWEST set that is complete in host memory — the last step's if its copy has landed, else the step's before
 * (*out_of_step = the internal step whose state they are; mi_world_get_step_mode_stats counts the same steps).  For a renderer that accepts one frame of latency — the
 * reference's own loop interpolates between the two last poses anyway (src/physics/physics.cpp:1395-1412): its next physicsStep then runs on the device while the rows of the
 * step it has not seen yet cross the bus, and a frame costs max(step, copy) instead of their sum.  The call never blocks except for the very first rows of a world.  What it
 * hands out stays intact until a stepping call produces into the same set: the rows of the step before the last are overwritten by the NEXT stepping call.  Read-only. */
MI_API int mi_world_view_transforms_landed(mi_world* world, uint32_t physics_transforms, const float** positions_xyz, const float** rotations_xyzw, uint32_t* out_count, uint64_t* out_of_step);
/* ... and the linear / angular velocities of every entity's rigid body (rigid_body_component::linearVelocity / angularVelocity; zero for an entity without one),
 * [count][3] each, out of the same rows: they ride along from the frame after the first request for velocities on (mi_world_get_velocities takes them from there too). */
MI_API int mi_world_view_velocities(mi_world* world, const float** linear_xyz, const float** angular_xyz, uint32_t* out_count);
MI_API int mi_world_get_velocities(mi_world* world, float* linear_xyz, float* angular_xyz, uint32_t capacity);
MI_API int mi_world_get_mass_properties(mi_world* world, float* inv_mass, float* inv_inertia_9, float* local_cog_xyz, uint32_t capacity);
MI_API int mi_world_get_counts(mi_world* world, mi_step_counts* out);
/* Contacts of the last internal step in solver (canonical) order; returns count in *out_count. */
MI_API int mi_world_get_contacts(mi_world* world, mi_contact* out, uint32_t capacity, uint32_t* out_count);
/* Diagnostics (no device needed): the tile -> XCD assignment of the XCD-partitioned contact solver for tile `tile_in_bin` of a
 * schedule bin with `tiles_in_bin` tiles: out[0] = owning XCD, out[1] = its rank inside that XCD's share of the bin,
 * out[2] = size of `query_xcd`'s share of the bin. */
MI_API int mi_debug_tile_owner(uint32_t tile_in_bin, uint32_t tiles_in_bin, uint32_t bin, uint32_t query_xcd, uint32_t* out);
/* Per-stage device times of the last internal step (HIP events on the world's stream).  Nothing is timed by default — even events attached to a
 * kernel's dispatch leave the device idle for a few microseconds (the solver's start / stop pair: ~11 us of a 1 ms step).  level 2: the whole step
 * (`total`) and the solve stage; level 3: the solve stage alone (`total` stays 0: the step's own start / stop events are two more such gaps — what bench.py runs its timed region
 * with, its roofline needs the solver launch's duration only); level 1: every stage (an event pair each); level 0: off. */
MI_API int mi_world_set_stage_timing(mi_world* world, uint32_t level);
MI_API int mi_world_get_stage_times(mi_world* world, mi_stage_times* out);
/* Contact-solver kernel of the last internal step: 0 k_contact_solve (a launch per colour per sweep), 1 k_contact_solve_flow,
 * 2 k_contact_solve_persist (default without joints), 3 k_solve_flow_islands (contacts + joint islands in one launch),
 * 4 k_contact_solve_persist with the tiles partitioned over the XCDs (default from 16384 manifolds up), 5 the same kernel with all
 * tiles on ONE XCD (default below that: every body hand-over through one L2). */
MI_API int mi_world_get_solver_kind(mi_world* world, uint32_t* out_kind);
/* Diagnostics: steps of a small scene whose enqueued work is bit-identical to that of a captured step are replayed as ONE HIP graph
 * (HIP runtime >= 7.2; MI_GRAPH=0 / force / all).  out[0] = enabled, out[1] = steps replayed, out[2] = graphs captured,
 * out[3] = speculative steps launched plainly. */
MI_API int mi_debug_step_graph_stats(mi_world* world, uint32_t* out4);
/* Tests: the device-wide exclusive prefix sum of the step (k_exclusive_scan) over a host array of `n` items of width_bits = 32 or 64 (64: two independent 32-bit sums side
 * by side, as the narrow phase packs them), run on the world's stream through the step's own scan sites (32: the cell histogram's, 64: the pair scan's), so behind the records,
 * tickets and generations that earlier steps and calls left there.  `out` receives the n prefix sums; zero_input != 0 asks the kernel to clear its input, and `in` then
 * receives the input array as the kernel left it.  No reference counterpart. */
MI_API int mi_debug_exclusive_scan(mi_world* world, uint32_t width_bits, void* in, uint32_t n, uint32_t zero_input, void* out);
/* Tests: in how many valid steps the colouring was finished by the tail inside k_bin_hist (the colouring rounds the host enqueued — what the previous step needed + 1 — left
 * manifolds uncoloured), and how many rounds ran there in total.  No reference counterpart (scheduleConstraintsSIMD is one serial pass, src/physics/constraints.cpp:51-184). */
MI_API int mi_debug_color_tail_stats(mi_world* world, uint64_t* out_steps, uint64_t* out_rounds);
/* Tests: how many times the pose rows (mi_world_view_transforms) were enqueued by a step itself, and how many times only when asked. */
MI_API int mi_debug_pose_stream_stats(mi_world* world, uint32_t* out_ahead, uint32_t* out_on_demand);
/* Step-ahead (no reference counterpart; what it takes off the path is the host's time between two physicsStep calls, src/physics/physics.cpp:1364-1413): a speculative step
 * enqueues the NEXT step's first kernel (world colliders + broad-phase classification) behind its own end-of-step record, into a second set of world-shape / AABB rows; the next step
 * adopts the result unless something its inputs depend on changed in between (a state write, an upload, another step mode, a void step).  How often it was enqueued / adopted. */
MI_API int mi_debug_step_ahead_stats(mi_world* world, uint64_t* out_enqueued, uint64_t* out_adopted);
/* Sum of the per-stage device times and of the contact updates (contacts x solver iterations) over the internal steps since
 * the last reset (so a benchmark loop does not have to call back into the library after every step). */
MI_API int mi_world_get_accumulated_stage_times(mi_world* world, mi_stage_times* out_sum, uint32_t* out_steps,
                                                uint64_t* out_contact_updates, uint32_t reset);
/* Stage dumps for parity bisecting: world AABBs (6 floats per collider, world index order) and the
 * solver colour of every manifold of the last step. */
MI_API int mi_world_get_aabbs(mi_world* world, float* out_min_max6, uint32_t capacity);
MI_API int mi_world_get_manifold_colors(mi_world* world, uint32_t* out_colors, uint32_t capacity);
/* Parity against the reference's own constraint order (debug speed: everything below runs sequentially).
 * PGS is order dependent; the library's canonical order is colour-major, the reference solves, per iteration, the joints of
 * every type in pool order and then the contacts in emission order (src/physics/constraints.cpp:3748-3770, 3381-3449).  These two calls make
 * the NEXT internal step follow what the caller says the reference did, so that a test can hold the library against the reference itself,
 * bit for bit, step after step:
 *   mi_debug_set_sweep_axis    the axis that step sweeps along (the reference picks it from float sums in pool order,
 *                              collision_broad.cpp:376-384, 443-444 — the library from an order-free integer statistic; they agree except
 *                              in near ties); later steps choose their own again
 *   mi_debug_set_solve_order   `pairs` = the oriented collider pairs (world indices A, B: 2 * count values) of the step's contact manifolds
 *                              in the order the reference emitted them.  The step then solves exactly these manifolds one after the other
 *                              in that order (one lane), the joints of each type one after the other in pool order, instead of the coloured
 *                              schedule; a manifold the step finds that is not in the list (or a listed one it does not find) makes the
 *                              step fail with MI_ERR_INVALID_ARGUMENT.  The list also ORIENTS pairs of equal shape type: where the AABB starts of
 *                              such a pair tie exactly on the sweep axis, the reference's (A, B) follows the history of its persistent endpoint
 *                              array (stable insertion sort, collision_broad.cpp:386-398), which no rule of the current state reproduces; a pair
 *                              listed the other way round is turned before the narrow phase.  Not with heightmap terrain or sharding
 *                              (MI_ERR_UNSUPPORTED). */
MI_API int mi_debug_set_sweep_axis(mi_world* world, uint32_t axis);
MI_API int mi_debug_set_solve_order(mi_world* world, const uint32_t* pairs, uint32_t count);
/*   mi_debug_set_solve_dataflow (sticky switch)  a step that follows a caller's order runs it through the PRODUCTION contact solver instead of the one-lane kernel: every
 *                              manifold is coloured with its level in the order's dependency graph (1 + the highest level among the earlier manifolds of its bodies),
 *                              so the colour-major dataflow schedule — bins, tiles, version bookkeeping, k_contact_solve_persist's tile code — performs the caller's
 *                              sequence of updates on every body: the caller's sequential result, bit for bit.  Needs an order at most 64 levels deep and no joints;
 *                              otherwise that step uses the one-lane kernel as before.  mi_debug_solve_order_depth: the depth the last such step ran with (0: it did not).
 *                              The reference's per-contact update it must reproduce: src/physics/constraints.cpp:3381-3449, its order 3748-3770.
 *   the colour history after an ordered step (either kernel): every manifold of that step enters the history with the overflow colour 64 — its key is kept
 *                              (collision begin / end events pair up as after any step), its colour is not: the next free step colours every manifold afresh
 *                              (greedy in descending pair priority, as for a world's first step), so the colours it solves in never mix the order's levels with
 *                              older colours.  mi_world_get_manifold_colors after an ordered step reports the colours that step ran with (levels, or 64). */
MI_API int mi_debug_set_solve_dataflow(mi_world* world, uint32_t enable);
MI_API int mi_debug_solve_order_depth(mi_world* world, uint32_t* out_depth);

/*
 * Cloth — cloth_component (src/physics/cloth.h:5-60, cloth.cpp): a gridSizeX x gridSizeY particle grid (upper row fixed) with
 * stretch / shear / bend distance constraints, stepped after the rigid bodies of every internal step
 * (physics.cpp:1352-1358): wind from the global force field, gravity, then numClothVelocityIterations /
 * numClothPositionIterations / numClothDriftIterations Gauss-Seidel passes (physics_settings defaults 0 / 1 / 0,
 * src/physics/physics.h:390-392; mi_world_set_cloth_iterations changes them).  Cloth does not interact with rigid bodies.
 *   mi_cloth_create             = cloth_component(width, height, gridSizeX, gridSizeY, totalMass, stiffness, damping, gravityFactor)
 *   mi_cloth_set_fixed_vertices = setWorldPositionOfFixedVertices(transform, moveRigid)
 *   mi_cloth_set_properties     = writing totalMass / stiffness / damping / gravityFactor (recalculateProperties on the next step)
 */
typedef struct mi_cloth_desc {
    float width, height;
    uint32_t grid_size_x, grid_size_y;
    float total_mass;
    float stiffness;        /* default 0.5 */
    float damping;          /* default 0.3 */
    float gravity_factor;   /* default 1 */
} mi_cloth_desc;
MI_API int mi_cloth_create(mi_world* world, const mi_cloth_desc* desc, uint32_t* out_cloth);
MI_API int mi_cloth_set_fixed_vertices(mi_world* world, uint32_t cloth, const float* position3, const float* rotation4, uint32_t move_rigid);
MI_API int mi_cloth_set_properties(mi_world* world, uint32_t cloth, float total_mass, float stiffness, float damping, float gravity_factor);
MI_API int mi_cloth_get_state(mi_world* world, uint32_t cloth, float* out_positions3, float* out_velocities3, uint32_t capacity_particles);
MI_API int mi_world_set_cloth_iterations(mi_world* world, uint32_t velocity_iterations, uint32_t position_iterations, uint32_t drift_iterations);

/*
 * Checkpoint / resume of the solver-relevant state: body states and accumulators, physics_transform0 and the
 * interpolated transforms, the step accumulator, the SAP axis of the next step, the contact-colour history (= the previous
 * step's collision list), the previous trigger overlaps, the constraint PODs.  A world built from the same scene description
 * that loads the blob continues bit-identically to the world that saved it.  save: out == NULL only reports the size.
 */
MI_API int mi_world_save_checkpoint(mi_world* world, void* out, uint64_t capacity, uint64_t* out_size);
MI_API int mi_world_load_checkpoint(mi_world* world, const void* data, uint64_t size);

/*
 * Collision events — collisionBeginCallback / collisionEndCallback of physics_settings (src/physics/physics.h:398-399),
 * fired by handleCollisionCallbacks (src/physics/physics.cpp:1041-1178).  The reference calls std::function callbacks
 * synchronously inside the step; across a C ABI they are polled: events of the internal steps since the last poll, per step
 * in ascending (collider_a, collider_b) order — the order of the reference's sorted merge of the previous and the current
 * frame's collision lists.  Like there, a pair is identified by its ORIENTED collider pair (a re-oriented pair ends and begins).
 * Disabled by default (the reference only diffs the lists when a callback is set); costs nothing when disabled.
 */
typedef enum mi_event_type {
    MI_EVENT_COLLISION_BEGIN = 0, MI_EVENT_COLLISION_END = 1,
    /* trigger_event_enter / trigger_event_leave (src/physics/physics.h:187-198): entity_a = the trigger entity, entity_b = the rigid
     * body's entity; de-duplicated per entity pair (several colliders may overlap), fired in ascending (trigger, body) order before
     * the collision events of the step, like handleNonCollisionInteractions (src/physics/physics.cpp:952-1039); colliders = ~0. */
    MI_EVENT_TRIGGER_ENTER = 2, MI_EVENT_TRIGGER_LEAVE = 3
} mi_event_type;
typedef struct mi_event {
    uint32_t type;                  /* mi_event_type */
    uint32_t entity_a, entity_b;    /* the colliders' parent entities (collision_begin_event::entityA/B) */
    uint32_t collider_a, collider_b;/* collider ids as returned by mi_collider_add (creation order) */
    float point[3];                 /* begin only: mean contact point, mean normal, velocity of B relative to A at the point */
    float normal[3];
    float relative_velocity[3];
} mi_event;
MI_API int mi_world_enable_events(mi_world* world, uint32_t enable);
MI_API int mi_world_poll_events(mi_world* world, mi_event* out, uint32_t capacity, uint32_t* out_count);

/*
 * Ghost-region exchange support (multi-GPU spatial sharding).  A body state is 13 floats:
 * position[3], rotation[4] (x,y,z,w), linear_velocity[3], angular_velocity[3] — i.e. physics_transform1 +
 * rigid_body_component velocities.  The host variants take entity ids and host buffers; the *_device variants
 * take rigid-body indices and state buffers that already live in this world's device memory (e.g. the
 * data_ptr() of torch CUDA tensors used with RCCL), so the exchange never round-trips through the host.
 */
#define MI_BODY_STATE_FLOATS 13
MI_API int mi_world_get_body_states(mi_world* world, uint32_t count, const uint32_t* entities, float* out_states13);
MI_API int mi_world_set_body_states(mi_world* world, uint32_t count, const uint32_t* entities, const float* states13);
MI_API int mi_world_entities_to_bodies(mi_world* world, uint32_t count, const uint32_t* entities, uint32_t* out_body_indices);
MI_API int mi_world_get_body_states_device(mi_world* world, uint32_t count, const uint32_t* body_indices_dev, float* out_states13_dev);
MI_API int mi_world_set_body_states_device(mi_world* world, uint32_t count, const uint32_t* body_indices_dev, const float* states13_dev);
/* The *_device calls without the host synchronisation: the copy kernels are only enqueued on the world's HIP stream
 * (mi_world_get_stream returns the hipStream_t).  Running the collective on that stream (torch.cuda.ExternalStream + RCCL) orders
 * gather -> exchange -> scatter -> next step on the device, with no host round trip in between. */
MI_API int mi_world_get_body_states_device_async(mi_world* world, uint32_t count, const uint32_t* body_indices_dev, float* out_states13_dev);
MI_API int mi_world_set_body_states_device_async(mi_world* world, uint32_t count, const uint32_t* body_indices_dev, const float* states13_dev);
MI_API int mi_world_get_stream(mi_world* world, void** out_hip_stream);

/*
 * Device-side access for a controller that lives on the same GPU (a policy in PyTorch, a sensor model, scripted pokes): motor targets in,
 * poses out, pushes and resets without a host copy.  Like the other *_device_async calls: the buffers are device memory (e.g. torch
 * tensors' data_ptr()), 16-byte aligned; the work is only ENQUEUED on the world's stream (mi_world_get_stream), no host synchronisation;
 * pending topology edits are uploaded first (that upload, like any, waits for the stream); a sharded world returns MI_ERR_UNSUPPORTED.
 * Two more cases wait for the stream, because the host still holds what the call needs: mi_constraints_update_device_async after a host
 * mi_constraint(s)_update that no step has sent up yet (it goes first), and mi_world_get_transforms_device_async while the host holds
 * the transforms (nothing stepped since the last download): they are sent up.  In a loop of device calls and steps neither occurs.  Each call leaves the world in the state its
 * host twin would: later steps, downloads and queries see no difference.
 */
/* The rows mi_world_get_transforms (physics_transforms = 0; the pending interpolation of mi_world_step included) or
 * mi_world_get_physics_transforms (!= 0) and mi_world_get_velocities would return at this point of the stream, byte for byte, in entity
 * order: positions [n][3], rotations [n][4], linear and angular velocities [n][3]; any pointer may be NULL.  Rows of entities WITHOUT a
 * rigid body are NOT WRITTEN: their transforms live on the host and never change in a step — fill them once from mi_world_get_transforms.
 * The pinned pose stream of mi_world_view_transforms is neither used nor disturbed. */
MI_API int mi_world_get_transforms_device_async(mi_world* world, uint32_t physics_transforms, float* positions3_dev, float* rotations4_dev,
                                                float* linear3_dev, float* angular3_dev);
/* Constraint ids -> positions in the type's device POD array (host side).  The positions stay valid until a constraint of that type is
 * created or destroyed. */
MI_API int mi_constraints_to_device_indices(mi_world* world, uint32_t type, uint32_t count, const uint32_t* constraint_ids, uint32_t* out_indices);
/* mi_constraints_update from device memory: whole PODs (pod_bytes = sizeof(mi_*_constraint) of the type, packed back to back) are written to
 * the positions indices_dev names (an index outside the array is skipped).  The device array is then newer than the library's host copy; the
 * library fetches it before mi_constraint_get reads that copy, before mi_constraint(s)_update / create / destroy change it, before a
 * topology upload re-sends it and before a checkpoint saves it — a later host update of one constraint keeps what the device wrote into the others. */
MI_API int mi_constraints_update_device_async(mi_world* world, uint32_t type, uint32_t count, const uint32_t* indices_dev, const void* pods_dev, uint32_t pod_bytes);
/* mi_world_test_interactions on rays in device memory: rays8_dev per ray origin3, direction3, strength, pad; ranges2_dev per ray the entity
 * range [lo, hi) it may hit, NULL = the whole scene.  Forces, torques and the order they are added in are those of the host call.  A ray with
 * an empty range (lo >= hi) hits nothing and costs no scan of the scene: a caller can keep one slot per environment and mark the idle ones so. */
MI_API int mi_world_test_interactions_device_async(mi_world* world, uint32_t count, const float* rays8_dev, const uint32_t* ranges2_dev);
/* mi_world_set_body_states_device_async where the device decides which rows count: row i is written iff mask_dev[i / group] != 0 (uint32
 * flags, one per `group` consecutive rows — e.g. one per environment of `group` bodies); every other body is left untouched. */
MI_API int mi_world_set_body_states_masked_device_async(mi_world* world, uint32_t count, const uint32_t* body_indices_dev, const float* states13_dev,
                                                        const uint32_t* mask_dev, uint32_t group);

#ifdef __cplusplus
}
#endif
#endif /* MI_PHYSICS_H */
