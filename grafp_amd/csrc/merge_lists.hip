// merge_lists.hip -- the `top` lists that the shards of a fingerprint library return for the same items, merged into one
// list per item (grafp_amd/sharded.py, ops.merge_track_lists), gfx950.
//
// Shard s of S <= 64 owns the global tracks [track_base[s], track_base[s + 1]) and has run an identify or match kernel
// (identify.hip, identify_thin.hip, identify_tempo.hip, crossmatch.hip, crossmatch_tempo.hip) on the global hit list
// minus its own row base: its list of an item is what the one-card kernel would rank, restricted to the shard's tracks,
// in the one-card order (score descending, then track ascending; local and global track numbers differ by a constant).
// The lists come in the form those kernels write: track int32 (S, n_items, top) with shard-local numbers, negative =
// padding; score f32 (S, n_items, top); the kernels' other outputs as n_payload <= 6 int32 arrays (n_payload, S, n_items,
// top), carried along unread.
// One workgroup per item: slot e = s * top + i holds entry i of shard s; its key is ~ord(score) << 32 | (track_base[s] +
// track), the empty key for padding.  The shards own disjoint tracks, so every key is unique, no per-track step is
// needed, and ONE block_sort (seqmatch.h) of (key, slot) ranks the S * top <= 4096 entries by score descending, then
// global track ascending -- the order of the producing kernels.  The first `top` go out as (n_items, top) track and
// score and (n_payload, n_items, top) payload, gathered through the slot; the rest of a list is padding: track -1, score
// -inf, payload p its own pad[p].  The merge is exact with lists of length top: a track ahead of t in the global order
// is either in another shard's list (and so in a slot) or ahead of t in t's own shard's list.
// crossmatch.hip marks a source that did not fit its workspace with track -2: if any entry of an item carries the mark,
// the item's slot 0 gets track -2 and everything else of the item is padding.
// track_base and pad travel in the kernel arguments (as TempoRatios does): nothing is copied, no host synchronisation,
// the launch goes out on the caller's stream and can be captured.  LDS: 10 bytes per slot, merge_slots(S, top) slots (at
// most 40 KiB).  Integer and bit moves only -- no float arithmetic, no atomics.
// Built WITHOUT packed-f32 instructions (Makefile NOPK), as identify_tempo.hip.
#include <climits>

#include "seqmatch.h"

namespace grafp {

constexpr int ML_THREADS = 256;
constexpr int ML_MAX_LISTS = 64, ML_MAX_TOP = 64, ML_MAX_SLOTS = 4096, ML_MAX_PAYLOAD = 6;
constexpr int ML_OVERFLOW = -2;                            // crossmatch.hip's mark of a source outside its workspace

struct MergeBases {
    int32_t base[ML_MAX_LISTS];                            // travels in the kernel arguments
};
struct MergePads {
    int32_t pad[ML_MAX_PAYLOAD];
};

__global__ __launch_bounds__(ML_THREADS) void merge_track_lists_kernel(
    MergeBases bases, MergePads pads, int S, int top, int n_payload, const int32_t *__restrict__ track,
    const float *__restrict__ score, const int32_t *__restrict__ payload, int32_t *__restrict__ out_track,
    float *__restrict__ out_score, int32_t *__restrict__ out_payload) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ml_smem[];       // 10 * P bytes (the launch's P)
    __shared__ int s_overflow;
    const int item = blockIdx.x, n_items = gridDim.x, tid = threadIdx.x;
    const int total = S * top;
    const int P = merge_slots(S, top);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ml_smem);
    unsigned short *idx = reinterpret_cast<unsigned short *>(ml_smem + (size_t)8 * P);
    if (tid == 0) s_overflow = 0;
    __syncthreads();
    // the input entry of merge slot e < total
    auto entry = [&](int e) -> size_t {
        const int s = e / top;
        return ((size_t)s * n_items + item) * top + (e - s * top);
    };
    for (int e = tid; e < P; e += ML_THREADS) {
        unsigned long long key = SEQ_NONE;
        if (e < total) {
            const size_t w = entry(e);
            const int t = track[w];
            if (t >= 0)
                key = ((unsigned long long)~f32_ord(score[w]) << 32) | (unsigned int)(bases.base[e / top] + t);
            else if (t == ML_OVERFLOW)
                s_overflow = 1;                            // (every writer stores the same value)
        }
        keys[e] = key;
        idx[e] = (unsigned short)e;
    }
    __syncthreads();
    block_sort<ML_THREADS, true>(keys, idx, P, tid);
    if (tid < top) {
        const unsigned long long key = s_overflow ? SEQ_NONE : keys[tid];         // top <= 64 <= P
        const size_t o = (size_t)item * top + tid, out_list = (size_t)n_items * top;
        if (key != SEQ_NONE) {
            const size_t w = entry(idx[tid]), in_list = (size_t)S * out_list;
            out_track[o] = (int)(key & 0xffffffffull);
            out_score[o] = ord_f32(~(unsigned int)(key >> 32));
            for (int p = 0; p < n_payload; ++p) out_payload[p * out_list + o] = payload[p * in_list + w];
        } else {
            out_track[o] = (s_overflow && tid == 0) ? ML_OVERFLOW : -1;
            out_score[o] = -INFINITY;
            for (int p = 0; p < n_payload; ++p) out_payload[p * out_list + o] = pads.pad[p];
        }
    }
}

int merge_track_lists_launch(const int32_t *track, const float *score, const int32_t *payload, int n_lists, int n_items,
                             int top, int n_payload, const int32_t *track_base, const int32_t *pad, int32_t *out_track,
                             float *out_score, int32_t *out_payload, hipStream_t stream) {
    GRAFP_REQUIRE(n_lists >= 1 && n_lists <= ML_MAX_LISTS, "merge_track_lists: n_lists=%d not in [1, %d]", n_lists,
                  ML_MAX_LISTS);
    GRAFP_REQUIRE(top >= 1 && top <= ML_MAX_TOP, "merge_track_lists: top=%d not in [1, %d]", top, ML_MAX_TOP);
    GRAFP_REQUIRE(n_lists * top <= ML_MAX_SLOTS, "merge_track_lists: %d lists x top=%d exceed the %d slots of the merge",
                  n_lists, top, ML_MAX_SLOTS);
    GRAFP_REQUIRE(n_payload >= 0 && n_payload <= ML_MAX_PAYLOAD, "merge_track_lists: n_payload=%d not in [0, %d]",
                  n_payload, ML_MAX_PAYLOAD);
    GRAFP_REQUIRE(n_items >= 0, "merge_track_lists: n_items=%d is negative", n_items);
    GRAFP_REQUIRE(track && score && track_base && out_track && out_score &&
                  (n_payload == 0 || (payload && pad && out_payload)), "merge_track_lists: null pointer");
    MergeBases bases = {};
    MergePads pads = {};
    for (int s = 0; s < n_lists; ++s) {
        GRAFP_REQUIRE(track_base[s] >= 0 && (s == 0 || track_base[s] >= track_base[s - 1]),
                      "merge_track_lists: track_base must be non-negative and ascending (track_base[%d]=%d)", s,
                      (int)track_base[s]);
        bases.base[s] = track_base[s];
    }
    for (int p = 0; p < n_payload; ++p) pads.pad[p] = pad[p];
    if (n_items == 0) return GRAFP_OK;
    hipLaunchKernelGGL(merge_track_lists_kernel, dim3(n_items), dim3(ML_THREADS), (size_t)10 * merge_slots(n_lists, top),
                       stream, bases, pads, n_lists, top, n_payload, track, score, payload, out_track, out_score,
                       out_payload);
    GRAFP_CHECK_LAUNCH("merge_track_lists_kernel");
    return GRAFP_OK;
}

}  // namespace grafp
