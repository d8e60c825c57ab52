// pcc_snapshot.h -- the format of a handle's snapshot (pcc_snapshot / pcc_restore, include/pcc_sim.h) and the launch functions of
// pcc_snapshot.hip.  No reference counterpart (the reference's env lives in one Python process and is never saved).
//
// A snapshot is one caller-owned device buffer:
//   header     SnapHeader: magic, version, the handle's configuration in clear and as a fingerprint, the host-side fields of
//              struct pcc_sim that steer the next step, where the ring regions of the snapshotted handle lie (SndBlk::ring_base
//              is a device address inside the state: restore rebases it region by region), the section table, and -- written by
//              the device, the host of pcc_snapshot never waits for them -- the number of live ring records and the bytes used;
//   verbatim   the small arrays as they are: the state blob's two runs (env and sender blocks with their shadows, refill rows,
//              restart statistics, class counts, cursors / any_done, pool stacks, history) and the work-list buffers;
//   rings      the in-flight rings COMPACTED: for every sender block (shadows included) the records [ha, ta) of its accepted ring,
//              then [hd, td) of its dropped ring, block after block -- nothing else of the rings (tier 0 alone is 24 KB a sender).
#pragma once
#include "pcc_dev.h"

namespace pcc {

constexpr uint64_t kSnapMagic = 0x3150414E53434350ull;   // "PCCSNAP1", little endian
constexpr uint32_t kSnapVersion = 1u;
constexpr int kSnapRegions = kMaxTiers + 1;   // where a ring_base can point: the tier blobs, then the shadows' private rings
enum { kSnapStateA = 0, kSnapStateB, kSnapLists, kSnapRings, kSnapSections };
constexpr uint32_t kSnapChunk = 1024;         // records of a ring one wavefront (its first chunk) or one workgroup (the others) moves

// What two handles must share to exchange snapshots; compared field by field (the message names the field) and as a hash
struct SnapConfig {
    int64_t n;
    int32_t ns, H, F, n_tiers;
    int32_t fid[kMaxFeatures];
    uint32_t ring_capacity, cap0, gid_base, parts;
    uint32_t tier_slots[kMaxTiers];
    int32_t rng_mode, use_cwnd, link_arrays, pad0;
    int64_t trace_stride;
    uint32_t key0, key1, max_steps, pad1;
    double delta_scale;
    double lo[5], hi[5];
};

// The host-side fields that steer the next step (struct pcc_sim, Dev)
struct SnapHost {
    uint32_t host_steps, step_seq, params_gen;
    int32_t read_buf, fill_buf, clean_buf, shadows;
    uint8_t lockstep, read_has_restarts, pad[2];
};

struct SnapSection { uint64_t offset, bytes; };

struct SnapHeader {
    uint64_t magic;
    uint32_t version, header_bytes;
    uint64_t fingerprint;
    SnapConfig cfg;
    SnapHost host;
    uint64_t region_base[kSnapRegions], region_bytes[kSnapRegions];
    SnapSection section[kSnapSections];   // (kSnapRings: its offset; its bytes are 16 * ring_records)
    // written by the device (snap_scan_kernel):
    uint64_t ring_records;   // live records stored
    uint64_t total_bytes;    // bytes of the snapshot = what pcc_snapshot_bytes returned
    uint32_t truncated;      // the buffer was too small for the records: none was stored, the snapshot is unusable
    uint32_t pad;
};
static_assert(sizeof(SnapHeader) % 8 == 0 && sizeof(SnapHeader) <= 1024, "the header is a kernel argument (the sections after it start 256-byte aligned)");

// source and target address of every ring region (a snapshot gathers with dst = src: the handle's own)
struct SnapRegions { uint64_t src[kSnapRegions], bytes[kSnapRegions], dst[kSnapRegions]; };

// the handle's scratch of the ring kernels: per tile of 64 rings the record count, then (scanned in place) its first record;
// control words; the rings longer than kSnapChunk
struct SnapScratch {
    unsigned long long *tile;    // [tiles]
    unsigned long long *total;   // [1] records of all rings
    uint32_t *ctl;               // [0] long rings listed, [1] skip: the records do not fit (or the header disagrees)
    ulonglong2 *longs;           // [rings] (first record, ring index)
};

inline int64_t snap_rings(const Dev &d) { return 2 * (int64_t)d.ns * d.stride; }   // an accepted and a dropped ring per sender block
inline int64_t snap_tiles(const Dev &d) { return (snap_rings(d) + kWave - 1) / kWave; }

// pcc_snapshot.hip
void launch_snap_header(const SnapHeader &h, void *buf, hipStream_t st);
// live records per tile of rings, their exclusive scan; total, truncation and (hdr != NULL) the header's device-written fields.
// restore: the counts come from the blocks just copied in; rings that break their bounds count 0 and flag their env
void launch_snap_count_scan(const Dev &d, const SnapRegions &r, const SnapScratch &s, SnapHeader *hdr, uint64_t ring_offset,
                            uint64_t room_records, uint64_t stated_records, bool restore, hipStream_t st);
// gather (restore = false: rings -> recs, nontemporal stores) or scatter (recs -> rings, plain stores), then on restore the rebase
// of every ring_base onto the target's regions
void launch_snap_move(const Dev &d, const SnapRegions &r, const SnapScratch &s, double2 *recs, bool restore, hipStream_t st);

}  // namespace pcc
