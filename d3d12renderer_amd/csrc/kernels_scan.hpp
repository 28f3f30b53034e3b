// kernels_scan.hpp — device-wide exclusive prefix sum (chained scan with decoupled look-back) and the pose rows for the caller.
// Part of the ONE translation unit of the physics library (world.hip includes kernels.hpp, which includes the stage files in pipeline order).
#pragma once   // (included by kernels.hpp only, after the stage files before it)

namespace mi {

// ------------------------------------------------------------------------------------------------------------------------------
// Device-wide exclusive prefix sum, ONE launch: chained scan with decoupled look-back.
//   * a workgroup takes its tile number from a ticket counter (so a tile's predecessors have always started), scans its
//     kScanTile items in registers / LDS and publishes first its AGGREGATE, then — after looking back over its predecessors'
//     records (one wave, kScanLookWindows x 64 records per round, until an inclusive prefix is found) — its INCLUSIVE PREFIX;
//   * a record is ONE aligned 16-byte granule (sum low word, sum high word, tag, tag), tag = generation << 2 | state (1 aggregate,
//     2 inclusive), written with one `sc1` (agent-scope, write-through) 16-byte store and read with one `sc1` 16-byte load, as the
//     contact solver's body granules are (kernels_solve.hpp): a reader that sees the tag sees the sum of the same store — no fences
//     (a release / acquire pair at agent scope would write back / invalidate the L2 around every record), no second load, no check
//     that two halves belong together;
//   * records are never reset: a reader ignores tags of older generations, and the ticket counter only ever grows
//     (`state[0]` = tickets handed out before this launch, `state[1]` = generation; the host clears everything long before the 30 generation bits wrap).
// T = uint32_t or a 64-bit word holding two independent 32-bit sums side by side (the narrow phase's packed
// (manifold flag, contact count); both totals stay below 2^32, so the halves never carry into each other).
constexpr uint32_t kScanThreads = 256;
// items per lane, measured per width (profiles/streaming_passes.txt): the 64-bit pair scan 9.8 us with 16 against 14.0 with 8 (twice the tiles, twice the tickets on one
// counter); the short 32-bit ones (cell histogram, schedule bins) 5.4 us with 8, 5.6 with 16, 6.0 with 4
constexpr uint32_t kScanItems64 = 16, kScanItems32 = 8;
template <typename T> struct ScanItems { static constexpr uint32_t N = sizeof(T) == 8 ? kScanItems64 : kScanItems32; static constexpr uint32_t Tile = kScanThreads * N; };
template <typename T> struct ScanWords { static constexpr uint32_t W = 2; };   // 64-bit words of one tile's record (the host sizes the record array with it)
constexpr uint32_t kScanLookWindows = 4;   // windows of 64 predecessors whose records one look-back round has in flight together
typedef uint32_t scan_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void scanPublish(scan_u32x4* rec, unsigned long long sum, uint32_t tag) {
    scan_u32x4 g; g.x = (uint32_t)sum; g.y = (uint32_t)(sum >> 32); g.z = tag; g.w = tag;
    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(rec), "v"(g) : "memory");
}
// kScanLookWindows records per lane, all in flight before the one wait
__device__ __forceinline__ void scanLoadRecords(const scan_u32x4* p0, const scan_u32x4* p1, const scan_u32x4* p2, const scan_u32x4* p3, scan_u32x4 (&g)[kScanLookWindows]) {
    static_assert(kScanLookWindows == 4, "one load per window below");
    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %5, off sc1\n\t"
                 "global_load_dwordx4 %2, %6, off sc1\n\tglobal_load_dwordx4 %3, %7, off sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]) : "v"(p0), "v"(p1), "v"(p2), "v"(p3) : "memory");
}
template <typename T>
__global__ __launch_bounds__(kScanThreads) void k_exclusive_scan(T* __restrict__ in, T* __restrict__ out, uint32_t n, unsigned long long* records,
                                                                 uint32_t* ticket, uint32_t* state /* [0] tickets handed out before this launch, [1] generation: kept ON THE DEVICE so that
                                                                 the launch has the same arguments every step (a captured HIP graph replays it) */, uint32_t zeroInput /* histograms: leave the input cleared for its next use */) {
    constexpr uint32_t kScanItems = ScanItems<T>::N, kScanTile = ScanItems<T>::Tile;
    constexpr uint32_t V = 16u / sizeof(T), NV = kScanItems / V;          // items of one 16-byte vector, vectors per lane
    static_assert(kScanItems % V == 0, "a lane owns whole 16-byte vectors");
    constexpr uint32_t kPitch = NV > 1 ? NV + 1 : 1;                        // a lane's NV vectors in LDS, plus one of padding: 16 lanes' 16-byte reads then fall on 64 different banks
    typedef T TV __attribute__((ext_vector_type(V)));
    __shared__ TV sData[kScanThreads * kPitch];
    __shared__ uint32_t sTile;
    __shared__ T sWave[kScanThreads / 64];
    __shared__ T sPrefix;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    __shared__ uint32_t sGen;
    if (tid == 0) {
        // the state is read BEFORE the ticket is taken (the ticket address depends on it), and only the workgroup holding the launch's
        // LAST ticket advances it — by then every other workgroup of the launch has taken its ticket, i.e. has read the state
        const uint32_t ticketBase = __hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t g = __hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t t = atomicAdd(ticket + ((ticketBase ^ g) >> 31 >> 1), 1u) - ticketBase;
        sTile = t; sGen = g;
        if (t == gridDim.x - 1u) {
            __hip_atomic_store(&state[0], ticketBase + gridDim.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[1], (g + 1u) & 0x3FFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    const uint32_t tile = sTile, gen = sGen;
    // Global memory is touched STRIPED: vector q = j * 256 + thread of the tile, so every load and store instruction of a wave covers one
    // contiguous 1 KB span (eight whole 128-byte lines).  The sum needs each thread's items consecutive (BLOCKED: thread t owns vectors
    // t * NV ..), so the tile crosses LDS once on the way in and once on the way out.  Blocked access to global memory (each thread reading its own
    // consecutive items) is correct too, but every lane then has its own 128-byte line and takes 16 bytes of it per instruction, and every line is
    // written eight times as a partial one: measured on the 64-bit pair scan (891 k items) 889 k write requests and 14.6 us against 112 k and 9.4 us
    // with this layout, the 32-bit scans 7.4 against 5.8 us (profiles/streaming_passes.txt).
    const size_t tileBase = (size_t)tile * kScanTile;
    const bool whole = tileBase + kScanTile <= (size_t)n;                                       // (workgroup-uniform, like the alignment tests)
    const bool vecIn = whole && ((uintptr_t)in & 15u) == 0u, vecOut = whole && ((uintptr_t)out & 15u) == 0u;   // callers' arrays (query offsets) need not be 16-byte aligned
    auto slot = [](uint32_t q) -> uint32_t { return NV > 1 ? q + q / NV : q; };
    {
        TV x[NV];
        if (vecIn) {
            const TV* src = reinterpret_cast<const TV*>(in + tileBase);
            #pragma unroll
            for (uint32_t j = 0; j < NV; ++j) x[j] = src[j * kScanThreads + tid];
            if (zeroInput) {
                TV* dst = reinterpret_cast<TV*>(in + tileBase);
                #pragma unroll
                for (uint32_t j = 0; j < NV; ++j) dst[j * kScanThreads + tid] = TV(0);
            }
        } else {
            #pragma unroll
            for (uint32_t j = 0; j < NV; ++j) {
                #pragma unroll
                for (uint32_t e = 0; e < V; ++e) { const size_t i = tileBase + (size_t)(j * kScanThreads + tid) * V + e; x[j][e] = i < n ? in[i] : T(0); }
            }
            if (zeroInput) {
                #pragma unroll
                for (uint32_t j = 0; j < NV; ++j) {
                    #pragma unroll
                    for (uint32_t e = 0; e < V; ++e) { const size_t i = tileBase + (size_t)(j * kScanThreads + tid) * V + e; if (i < n) in[i] = T(0); }
                }
            }
        }
        #pragma unroll
        for (uint32_t j = 0; j < NV; ++j) sData[slot(j * kScanThreads + tid)] = x[j];
    }
    __syncthreads();
    T v[kScanItems];
    #pragma unroll
    for (uint32_t j = 0; j < NV; ++j) {
        const TV x = sData[tid * kPitch + j];
        #pragma unroll
        for (uint32_t e = 0; e < V; ++e) v[j * V + e] = x[e];
    }
    T local = 0;
    #pragma unroll
    for (uint32_t k = 0; k < kScanItems; ++k) { T x = v[k]; v[k] = local; local += x; }      // exclusive within the thread
    T incl = local;                                                                         // inclusive across the wave
    #pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) { T o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    if (lane == 63u) sWave[wave] = incl;
    __syncthreads();
    T waveOff = 0, aggregate = 0;
    #pragma unroll
    for (uint32_t w = 0; w < kScanThreads / 64; ++w) { if (w < wave) waveOff += sWave[w]; aggregate += sWave[w]; }
    {   // exclusive within the tile, back into the thread's own LDS vectors (nobody else reads or writes them before the barrier below)
        const T off = waveOff + (incl - local);
        #pragma unroll
        for (uint32_t j = 0; j < NV; ++j) {
            TV x;
            #pragma unroll
            for (uint32_t e = 0; e < V; ++e) x[e] = off + v[j * V + e];
            sData[tid * kPitch + j] = x;
        }
    }
    if (wave == 0) {
        T prefix = 0;
        const uint32_t tagAgg = (gen << 2) | 1u, tagInc = (gen << 2) | 2u;
        scan_u32x4* recs = reinterpret_cast<scan_u32x4*>(records);
        if (tile == 0) {
            if (lane == 0) scanPublish(recs, (unsigned long long)aggregate, tagInc);
        } else {
            if (lane == 0) scanPublish(recs + tile, (unsigned long long)aggregate, tagAgg);
            int32_t look = (int32_t)tile - 1;
            while (true) {                                   // kScanLookWindows x 64 predecessors per round, nearest first; rounds never overlap
                T val[kScanLookWindows]; uint32_t st[kScanLookWindows]; const scan_u32x4* rp[kScanLookWindows];
                #pragma unroll
                for (uint32_t k = 0; k < kScanLookWindows; ++k) {
                    const int32_t idx = look - (int32_t)(k * 64u + lane);
                    val[k] = 0; st[k] = idx < 0 ? 3u : 0u;                     // 3: before the first tile (contributes nothing, ends the search)
                    rp[k] = recs + (idx < 0 ? 0 : idx);
                }
                T contrib; bool found;
                while (true) {
                    scan_u32x4 g[kScanLookWindows];
                    scanLoadRecords(rp[0], rp[1], rp[2], rp[3], g);
                    #pragma unroll
                    for (uint32_t k = 0; k < kScanLookWindows; ++k)
                        if (st[k] == 0u && (g[k].z == tagAgg || g[k].z == tagInc)) {      // a publication of this generation (a record taken earlier is not taken again)
                            st[k] = g[k].z & 3u;
                            val[k] = (T)(((unsigned long long)g[k].y << 32) | (unsigned long long)g[k].x);
                        }
                    // window by window, nearest first: everything nearer than (and including) the first inclusive record must have arrived
                    contrib = 0; found = false; bool pending = false;
                    #pragma unroll
                    for (uint32_t k = 0; k < kScanLookWindows; ++k) {
                        if (found || pending) continue;
                        const unsigned long long done = __ballot(st[k] >= 2u), wait = __ballot(st[k] == 0u);
                        const uint32_t first = done ? (uint32_t)__ffsll((long long)done) - 1u : 63u;
                        const unsigned long long need = first >= 63u ? ~0ull : (2ull << first) - 1ull;
                        if (wait & need) pending = true;
                        else { if ((need >> lane) & 1ull) contrib += val[k]; found = done != 0ull; }
                    }
                    if (!pending) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                #pragma unroll
                for (uint32_t d = 32; d >= 1; d >>= 1) contrib += __shfl_xor(contrib, d, 64);
                prefix += contrib;
                if (found) break;
                look -= (int32_t)(64u * kScanLookWindows);
            }
            if (lane == 0) scanPublish(recs + tile, (unsigned long long)(prefix + aggregate), tagInc);
        }
        if (lane == 0) sPrefix = prefix;
    }
    __syncthreads();
    const T prefix = sPrefix;
    if (vecOut) {
        TV* dst = reinterpret_cast<TV*>(out + tileBase);
        #pragma unroll
        for (uint32_t j = 0; j < NV; ++j) dst[j * kScanThreads + tid] = sData[slot(j * kScanThreads + tid)] + TV(prefix);
    } else {
        #pragma unroll
        for (uint32_t j = 0; j < NV; ++j) {
            const TV x = sData[slot(j * kScanThreads + tid)];
            #pragma unroll
            for (uint32_t e = 0; e < V; ++e) { const size_t i = tileBase + (size_t)(j * kScanThreads + tid) * V + e; if (i < n) out[i] = prefix + x[e]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------ poses for the caller
// The transforms the caller reads after a step (transform_component of every entity with a rigid body), produced where the bodies live:
// one lane per entity, out as [n][3] positions followed by [n][4] rotations — the layout of mi_world_get_transforms — so that ONE
// device-to-host copy of 28 B per entity follows instead of 2-4 arrays of 16 B per body and a host pass over them.
// lerpT < 0: transform = physics_transform1 (physics.cpp:1408-1411); else lerp(transform0, transform1, t), nlerp on the rotation
// (physics.cpp:1392-1406, src/core/math.h:673-682) — the same expressions as the host path (download()), bit for bit.
// Entities without a rigid body keep their host-side transform: their rows are left alone here and filled in by the host.
__global__ __launch_bounds__(256) void k_entity_poses(uint32_t n, const int* __restrict__ entBody, const float4* __restrict__ pos, const float4* __restrict__ rot,
                                                      const float4* __restrict__ pos0, const float4* __restrict__ rot0, float lerpT, float* __restrict__ outP, float* __restrict__ outR,
                                                      const float4* __restrict__ lin, const float4* __restrict__ ang, float* __restrict__ outL, float* __restrict__ outA /* [n][3] each, or null: the velocities ride along */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = entBody[i];
    if (b < 0) return;
    if (outL) {
        const float4 l = lin[b], a = ang[b];
        outL[3 * (size_t)i] = l.x; outL[3 * (size_t)i + 1] = l.y; outL[3 * (size_t)i + 2] = l.z;
        outA[3 * (size_t)i] = a.x; outA[3 * (size_t)i + 1] = a.y; outA[3 * (size_t)i + 2] = a.z;
    }
    const float4 p1 = pos[b], r1 = rot[b];
    V3 ps(p1.x, p1.y, p1.z); Q4 rt(r1.x, r1.y, r1.z, r1.w);
    if (lerpT >= 0.f) {
        const float4 p0 = pos0[b], r0 = rot0[b]; const float t = lerpT;
        ps = lerp(V3(p0.x, p0.y, p0.z), ps, t);
        rt = normalize(Q4(r0.x + t * (r1.x - r0.x), r0.y + t * (r1.y - r0.y), r0.z + t * (r1.z - r0.z), r0.w + t * (r1.w - r0.w)));
    }
    outP[3 * (size_t)i] = ps.x; outP[3 * (size_t)i + 1] = ps.y; outP[3 * (size_t)i + 2] = ps.z;
    *reinterpret_cast<float4*>(outR + 4 * (size_t)i) = make_float4(rt.x, rt.y, rt.z, rt.w);
}

}  // namespace mi
