// pcc_snapshot.hip -- the device side of pcc_snapshot / pcc_restore (include/pcc_sim.h; the format: pcc_snapshot.h): the in-flight
// rings of a handle gathered into, or scattered from, one dense run of 16-byte records.  No reference counterpart.
//
// A ring's live records [head, tail) are a contiguous run modulo the ring's capacity; there are two rings per sender block (and as
// many again for the shadows), a few hundred records in most, ~100 000 in a tier-3 ring of a saturated link.  Four kernels:
//   snap_count_kernel   a lane per ring: live records (0 for a ring that breaks its bounds), summed per tile of 64 rings;
//   snap_scan_kernel    one workgroup: the exclusive scan over the tiles, the total, and the header's device-written fields;
//   snap_move_kernel    a wavefront per tile: the scan inside the tile, then ring after ring the first kSnapChunk records, 64
//                       consecutive records per instruction (1 KB of consecutive bytes on both sides up to the ring's wrap), four
//                       instructions in flight; a longer ring is listed;
//   snap_move_long_kernel  a workgroup per further chunk of a listed ring (block x = chunk, block y strides over the list): a
//                       tier-3 ring is moved by as many workgroups as it has chunks, never by one wavefront.
// Ring reads are plain loads; the gather's stores into the snapshot are dense and nontemporal (st_rec_nt: nobody reads them soon);
// the scatter writes the rings with ordinary stores (the retire half reads them next).  On restore snap_rebase_kernel then moves
// every SndBlk::ring_base from the snapshotted handle's regions onto the target's.
// Bounds (a bad buffer must never become a stray write): a ring is moved only if its tier exists, its record count fits its
// capacity, its storage lies inside ONE region of the handle and its records inside the snapshot's record section; otherwise
// nothing of it is written and (restore) its env gets PCC_FLAG_INTERNAL.
#include "pcc_snapshot.h"

namespace {

struct SnapRing {
    uint64_t ptr;    // first slot of the ring (target address)
    uint32_t mask, head, cnt;
    uint32_t bad;
};

// address p (of `len` bytes, in the snapshotted handle) -> the same place in the target's region; false: in no region
__device__ __forceinline__ bool snap_translate(const SnapRegions &R, const uint64_t p, const uint64_t len, uint64_t &out) {
    bool in = false;
#pragma unroll
    for (int q = 0; q < kSnapRegions; q++) {
        const bool here = R.bytes[q] != 0 && R.dst[q] != 0 && p >= R.src[q] && p - R.src[q] <= R.bytes[q] && len <= R.bytes[q] - (p - R.src[q]);
        if (here && !in) { in = true; out = R.dst[q] + (p - R.src[q]); }
    }
    return in && (p & 15u) == 0;   // (records are 16-byte aligned)
}

__device__ __forceinline__ bool snap_tier_cap(const Dev &D, const uint32_t tier, uint32_t &cap) {
    const bool ok = tier < (uint32_t)D.n_tiers || (tier == kTierBorrowed && D.n_tiers >= 2);
    cap = ok ? tier_cap(D, tier) : 0u;
    return ok;
}

// ring r = 2 * sender block + (0: accepted, 1: dropped), its live run as target addresses; cnt = 0 for an empty or a bad ring
__device__ __forceinline__ SnapRing snap_ring(const Dev &D, const SnapRegions &R, const int64_t r, const int64_t rings) {
    SnapRing g = {0ull, 0u, 0u, 0u, 0u};
    if (r >= rings) return g;
    const SndBlk *b = D.snd + (r >> 1);
    const bool dropped = (r & 1) != 0;
    const uint32_t head = dropped ? b->hd : b->ha, cnt = (dropped ? b->td : b->ta) - head;
    if (cnt == 0u) return g;
    uint32_t cap = 0;
    const bool tier_ok = snap_tier_cap(D, b->ring_tier, cap);
    const uint32_t room = dropped ? 2u * cap : cap;
    const uint64_t p = reinterpret_cast<uint64_t>(b->ring_base), len = (uint64_t)3 * cap * sizeof(double2);
    uint64_t base = 0;
    const bool in = snap_translate(R, p, len, base);
    if (!tier_ok || cnt > room || !in) { g.bad = 1u; return g; }
    g.ptr = base + (dropped ? (uint64_t)cap * sizeof(double2) : 0ull);
    g.mask = room - 1u;
    g.head = head;
    g.cnt = cnt;
    return g;
}

__device__ __forceinline__ void snap_flag(const Dev &D, const int64_t k /* sender block */) {
    atomicOr(&D.env[env_of(D, k % D.stride)].flags, PCC_FLAG_INTERNAL);
}

__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v, const uint32_t lane) {
#pragma unroll
    for (uint32_t o = 1; o < (uint32_t)kWave; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(256) void snap_count_kernel(Dev D, SnapRegions R, SnapScratch S, int64_t rings, int64_t tiles, int restore) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const SnapRing g = snap_ring(D, R, r, rings);
    if (g.bad && restore) snap_flag(D, r >> 1);
    unsigned long long c = g.cnt;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63u) == 0u && (r >> 6) < tiles) S.tile[r >> 6] = c;
}

// one workgroup: tile counts -> first record of every tile; the total; whether the records fit (and, on restore, are as many as the header says)
__global__ __launch_bounds__(1024) void snap_scan_kernel(Dev D, SnapScratch S, int64_t tiles, SnapHeader *hdr, uint64_t ring_offset,
                                                         uint64_t room_records, uint64_t stated_records, int restore) {
    __shared__ unsigned long long wsum[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < tiles; base += 1024) {
        const int64_t j = base + t;
        const unsigned long long v = j < tiles ? S.tile[j] : 0ull;
        const unsigned long long inc = wave_inclusive_scan(v, lane);
        if (lane == 63u) wsum[w] = inc;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (uint32_t q = 0; q < 16u; q++) {
            const unsigned long long x = wsum[q];
            before += q < w ? x : 0ull;
            all += x;
        }
        if (j < tiles) S.tile[j] = carry + before + inc - v;
        carry += all;
        __syncthreads();
    }
    if (t == 0u) {
        const bool skip = carry > room_records || (restore && carry != stated_records);
        *S.total = carry;
        S.ctl[0] = 0u;
        S.ctl[1] = skip ? 1u : 0u;
        if (hdr) {
            hdr->ring_records = carry;
            hdr->total_bytes = ring_offset + carry * sizeof(double2);
            hdr->truncated = carry > room_records ? 1u : 0u;
        }
        if (restore && skip) atomicOr(&D.env[0].flags, PCC_FLAG_INTERNAL);   // (the host checked the header: only a payload that disagrees with it gets here)
    }
}

// n records of a run: ring slots (head + j) & mask <-> recs[j], j = 0 .. n-1, by `threads` threads (this one: t), kDepth instructions in flight
template <bool kRestore>
__device__ __forceinline__ void snap_move_run(double2 *ring, const uint32_t mask, const uint32_t head, double2 *recs, const uint32_t n,
                                              const uint32_t t, const uint32_t threads) {
    constexpr int kDepth = 4;
    for (uint32_t j0 = 0; j0 < n; j0 += kDepth * threads) {
        double2 v[kDepth];
#pragma unroll
        for (int b = 0; b < kDepth; b++) {
            const uint32_t j = j0 + (uint32_t)b * threads + t;
            v[b].x = 0.0; v[b].y = 0.0;
            if (j < n) v[b] = ld_rec(kRestore ? recs + j : ring + ((head + j) & mask));
        }
#pragma unroll
        for (int b = 0; b < kDepth; b++) {
            const uint32_t j = j0 + (uint32_t)b * threads + t;
            if (j < n) {
                if (kRestore) st_rec(ring + ((head + j) & mask), v[b]);
                else st_rec_nt(recs + j, v[b]);
            }
        }
    }
}

template <bool kRestore>
__global__ __launch_bounds__(256) void snap_move_kernel(Dev D, SnapRegions R, SnapScratch S, double2 *recs, int64_t rings, int64_t tiles) {
    if (S.ctl[1]) return;
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= tiles) return;
    const int64_t r = tile * kWave + lane;
    const SnapRing g = snap_ring(D, R, r, rings);
    const unsigned long long first = S.tile[tile] + wave_inclusive_scan(g.cnt, lane) - g.cnt;
    if (g.cnt > kSnapChunk) S.longs[atomicAdd(&S.ctl[0], 1u)] = make_ulonglong2(first, (unsigned long long)r);
    uint64_t live = __ballot(g.cnt != 0u);
    while (live) {
        const uint32_t l = (uint32_t)__ffsll((unsigned long long)live) - 1u;
        live &= live - 1ull;
        const uint32_t cnt = rl_u32(g.cnt, l);
        snap_move_run<kRestore>(reinterpret_cast<double2 *>(rl_u64(g.ptr, l)), rl_u32(g.mask, l), rl_u32(g.head, l), recs + rl_u64(first, l),
                                cnt < kSnapChunk ? cnt : kSnapChunk, lane, kWave);
    }
}

// chunk blockIdx.x + 1 of every listed ring that has one
template <bool kRestore>
__global__ __launch_bounds__(256) void snap_move_long_kernel(Dev D, SnapRegions R, SnapScratch S, double2 *recs, int64_t rings) {
    if (S.ctl[1]) return;
    const uint32_t n_long = S.ctl[0];
    const uint64_t begin = ((uint64_t)blockIdx.x + 1u) * kSnapChunk;
    for (uint32_t li = blockIdx.y; li < n_long; li += gridDim.y) {
        const ulonglong2 e = S.longs[li];
        const SnapRing g = snap_ring(D, R, (int64_t)e.y, rings);
        if (begin >= g.cnt) continue;
        const uint32_t left = g.cnt - (uint32_t)begin;
        snap_move_run<kRestore>(reinterpret_cast<double2 *>(g.ptr), g.mask, g.head + (uint32_t)begin, recs + e.x + begin,
                                left < kSnapChunk ? left : kSnapChunk, threadIdx.x, 256u);
    }
}

// restore, last: every ring_base from the snapshotted handle's regions onto this handle's.  A block whose rings lie in no region
// (only a tampered payload) is emptied into storage of its own and its env flagged: no foreign address stays in the state
__global__ __launch_bounds__(256) void snap_rebase_kernel(Dev D, SnapRegions R) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (int64_t)D.ns * D.stride) return;
    SndBlk *b = D.snd + k;
    const uint64_t p = reinterpret_cast<uint64_t>(b->ring_base);
    if (!p) return;   // (a shadow that was never prepared)
    uint32_t cap = 0;
    const bool tier_ok = snap_tier_cap(D, b->ring_tier, cap);
    const uint64_t len = (uint64_t)3 * cap * sizeof(double2);
    uint64_t base = 0;
    const bool in = snap_translate(R, p, len, base);
    if (tier_ok && in) { b->ring_base = reinterpret_cast<char *>(base); return; }
    const int64_t s = k / D.stride, i = k % D.stride;
    snap_flag(D, k);
    b->ha = b->ta; b->hd = b->td;
    if (i < D.n) {
        b->ring_tier = 0;
        b->ring_base = D.tier_base[0] + (size_t)(i * D.ns + s) * tier_slot_bytes(D, 0);
    } else {
        b->ring_base = nullptr;
        D.env[i].resetting = 3;   // (unusable: the env restarts through the restart list, and the shadow is prepared again from there)
    }
}

__global__ void snap_header_kernel(SnapHeader h, SnapHeader *dst) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = h;
}

}  // namespace

namespace pcc {

void launch_snap_header(const SnapHeader &h, void *buf, hipStream_t st) {
    hipLaunchKernelGGL(snap_header_kernel, dim3(1), dim3(kWave), 0, st, h, static_cast<SnapHeader *>(buf));
}

void launch_snap_count_scan(const Dev &d, const SnapRegions &r, const SnapScratch &s, SnapHeader *hdr, uint64_t ring_offset,
                            uint64_t room_records, uint64_t stated_records, bool restore, hipStream_t st) {
    const int64_t rings = snap_rings(d), tiles = snap_tiles(d);
    hipLaunchKernelGGL(snap_count_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, d, r, s, rings, tiles, restore ? 1 : 0);
    hipLaunchKernelGGL(snap_scan_kernel, dim3(1), dim3(1024), 0, st, d, s, tiles, hdr, ring_offset, room_records, stated_records, restore ? 1 : 0);
}

void launch_snap_move(const Dev &d, const SnapRegions &r, const SnapScratch &s, double2 *recs, bool restore, hipStream_t st) {
    const int64_t rings = snap_rings(d), tiles = snap_tiles(d);
    const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
    // chunks of the largest ring there is (a dropped ring of the top tier) beyond the first; the list is walked by as many rows
    // of workgroups as keep the launch below ~64 K workgroups
    const uint64_t top = (uint64_t)2 * ((uint64_t)d.cap0 << (2 * (d.n_tiers - 1)));
    const uint64_t more = top > kSnapChunk ? (top + kSnapChunk - 1) / kSnapChunk - 1 : 0;
    uint64_t rows = more ? 65536 / more : 0;
    rows = rows < 1 ? 1 : rows > 64 ? 64 : rows;
    const dim3 long_grid((unsigned)more, (unsigned)rows);
    if (restore) {
        hipLaunchKernelGGL(snap_move_kernel<true>, grid, block, 0, st, d, r, s, recs, rings, tiles);
        if (more) hipLaunchKernelGGL(snap_move_long_kernel<true>, long_grid, block, 0, st, d, r, s, recs, rings);
        hipLaunchKernelGGL(snap_rebase_kernel, dim3((unsigned)((rings / 2 + 255) / 256)), block, 0, st, d, r);
    } else {
        hipLaunchKernelGGL(snap_move_kernel<false>, grid, block, 0, st, d, r, s, recs, rings, tiles);
        if (more) hipLaunchKernelGGL(snap_move_long_kernel<false>, long_grid, block, 0, st, d, r, s, recs, rings);
    }
}

}  // namespace pcc
