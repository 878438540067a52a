// srlx_seqstore.hip -- Agent57's sequence replay in HBM (include/srlx.h, "Agent57 sequence store"): one launch assembles a sampled batch of sequences from the
// frame ring and the per-sequence records into the tensors the trainer feeds its networks.  The kernel moves data and computes nothing: no atomics, no LDS, no
// scratch.  Rows are copied with 16-byte accesses when the frame length allows it and with dword accesses otherwise; the path is a property of the launch.
#include "srlx_common.h"

namespace {

using i64 = long long;
using u8 = unsigned char;

constexpr int kThreads = 256;
constexpr int kInFlight = 4;                      // loads a lane issues before its first store
constexpr int kChunk = kThreads * kInFlight;      // copy units (float4 or float) one workgroup moves

struct SeqGatherArgs {
    i64 B;
    int L, S, A, H;
    i64 frame_elems, frame_stride, frame_capacity, seq_capacity, record_stride;
    const int64_t *slots;
    const float *ring;
    const int32_t *records;
    float *states;
    int64_t *actions;
    float *r_ext, *r_int, *dones;
    u8 *invalid;
    int64_t *actor;
    float *h_ext, *c_ext, *h_int, *c_int;
};

template <typename V>
__device__ __forceinline__ V zero_of();
template <>
__device__ __forceinline__ float zero_of<float>() {
    return 0.f;
}
template <>
__device__ __forceinline__ float4 zero_of<float4>() {
    return make_float4(0.f, 0.f, 0.f, 0.f);
}

// workgroups [0, B L) x chunks: frame l of batch row b; workgroups [B L, B L + B) (chunk 0 only): the small fields of batch row b
template <typename V>
__global__ __launch_bounds__(kThreads) void k_seq_gather(SeqGatherArgs a) {
    const i64 row = blockIdx.x;
    const i64 n_frames = a.B * a.L;
    const int tid = threadIdx.x;
    if (row < n_frames) {
        const i64 b = row / a.L;
        const int l = (int)(row - b * a.L);
        const i64 s = a.slots[b];
        i64 f = -1;
        if (s >= 0 && s < a.seq_capacity) f = a.records[s * a.record_stride + l];
        const bool zero = f < 0 || f >= a.frame_capacity;  // -1: an all-zero frame; anything else outside the ring is never dereferenced
        constexpr int kPer = (int)(sizeof(V) / sizeof(float));
        const i64 units = a.frame_elems / kPer;  // (the vector path runs only when frame_elems is a multiple of 4)
        const V *src = (const V *)(a.ring + (zero ? 0 : f) * a.frame_stride);
        V *dst = (V *)(a.states + row * a.frame_elems);
        const i64 base = (i64)blockIdx.y * kChunk + tid;
        V v[kInFlight];
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            v[k] = zero_of<V>();
            if (!zero && i < units) v[k] = src[i];
        }
#pragma unroll
        for (int k = 0; k < kInFlight; ++k) {
            const i64 i = base + (i64)k * kThreads;
            if (i < units) dst[i] = v[k];
        }
        return;
    }
    if (blockIdx.y != 0) return;
    const i64 b = row - n_frames;
    const i64 s = a.slots[b];
    const bool live = s >= 0 && s < a.seq_capacity;
    const int32_t *rec = a.records + (live ? s : 0) * a.record_stride;
    const int L = a.L, S = a.S, A = a.A, H = a.H;
    const int32_t *rec_act = rec + L;
    const float *rec_rext = (const float *)(rec + 2 * L), *rec_rint = (const float *)(rec + 3 * L), *rec_undone = (const float *)(rec + 4 * L);
    const float *rec_hid = (const float *)(rec + 4 * L + S + 1);
    const u8 *rec_inv = (const u8 *)(rec + 4 * L + S + 1 + 4 * H);
    for (int i = tid; i < L; i += kThreads) {
        a.actions[b * L + i] = live ? (int64_t)rec_act[i] : 0;
        a.r_ext[b * L + i] = live ? rec_rext[i] : 0.f;
        a.r_int[b * L + i] = live ? rec_rint[i] : 0.f;
    }
    for (int i = tid; i < S; i += kThreads) a.dones[b * S + i] = live ? rec_undone[i] : 0.f;
    for (int i = tid; i < S * A; i += kThreads) a.invalid[b * (i64)S * A + i] = live ? rec_inv[i] : (u8)0;
    if (tid == 0) a.actor[b] = live ? (int64_t)rec[4 * L + S] : 0;
    for (int i = tid; i < H; i += kThreads) {
        a.h_ext[b * H + i] = live ? rec_hid[i] : 0.f;
        a.c_ext[b * H + i] = live ? rec_hid[H + i] : 0.f;
        a.h_int[b * H + i] = live ? rec_hid[2 * H + i] : 0.f;
        a.c_int[b * H + i] = live ? rec_hid[3 * H + i] : 0.f;
    }
}

bool in_envelope(int64_t L, int64_t S, int64_t A, int64_t H) {
    return L >= 2 && L <= SRLX_SEQ_MAX_L && S >= 1 && S < L && A >= 1 && A <= SRLX_SEQ_MAX_A && H >= 1 && H <= SRLX_SEQ_MAX_H;
}

i64 record_dwords(int64_t L, int64_t S, int64_t A, int64_t H) { return (4 * L + S + 1 + 4 * H + (S * A + 3) / 4 + 3) / 4 * 4; }

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t srlx_seq_record_dwords(int64_t L, int64_t S, int64_t A, int64_t H) { return in_envelope(L, S, A, H) ? record_dwords(L, S, A, H) : -1; }

int srlx_seq_gather(int64_t B, int64_t L, int64_t S, int64_t A, int64_t H, int64_t frame_elems, int64_t frame_stride, int64_t frame_capacity, int64_t seq_capacity,
                    int64_t record_stride, const int64_t *d_slots, const float *d_ring, const int32_t *d_records, float *d_states, int64_t *d_actions,
                    float *d_r_ext, float *d_r_int, float *d_dones, uint8_t *d_invalid, int64_t *d_actor, float *d_h_ext, float *d_c_ext, float *d_h_int,
                    float *d_c_int, void *stream) {
    SRLX_REQUIRE(B >= 1 && B <= SRLX_SEQ_MAX_B, "srlx_seq_gather: batch %lld outside 1..%d", (long long)B, SRLX_SEQ_MAX_B);
    SRLX_REQUIRE(L >= 2 && L <= SRLX_SEQ_MAX_L, "srlx_seq_gather: window L %lld outside 2..%d", (long long)L, SRLX_SEQ_MAX_L);
    SRLX_REQUIRE(S >= 1 && S < L, "srlx_seq_gather: sequence length S %lld must be in 1..L-1 (L %lld)", (long long)S, (long long)L);
    SRLX_REQUIRE(A >= 1 && A <= SRLX_SEQ_MAX_A, "srlx_seq_gather: actions A %lld outside 1..%d", (long long)A, SRLX_SEQ_MAX_A);
    SRLX_REQUIRE(H >= 1 && H <= SRLX_SEQ_MAX_H, "srlx_seq_gather: recurrent units H %lld outside 1..%d", (long long)H, SRLX_SEQ_MAX_H);
    SRLX_REQUIRE(frame_elems >= 1 && frame_elems <= SRLX_SEQ_MAX_FRAME_ELEMS, "srlx_seq_gather: frame_elems %lld outside 1..%d", (long long)frame_elems,
                 SRLX_SEQ_MAX_FRAME_ELEMS);
    SRLX_REQUIRE(frame_stride >= frame_elems, "srlx_seq_gather: frame_stride %lld below frame_elems %lld", (long long)frame_stride, (long long)frame_elems);
    SRLX_REQUIRE(frame_capacity >= 1 && frame_capacity <= SRLX_SEQ_MAX_FRAME_CAPACITY, "srlx_seq_gather: frame_capacity %lld outside 1..2^31-1",
                 (long long)frame_capacity);
    SRLX_REQUIRE(seq_capacity >= 1, "srlx_seq_gather: seq_capacity %lld must be positive", (long long)seq_capacity);
    SRLX_REQUIRE(record_stride >= record_dwords(L, S, A, H), "srlx_seq_gather: record_stride %lld below the record's %lld dwords", (long long)record_stride,
                 (long long)record_dwords(L, S, A, H));
    SRLX_REQUIRE(d_slots && d_ring && d_records, "srlx_seq_gather: an input pointer is NULL");
    SRLX_REQUIRE(d_states && d_actions && d_r_ext && d_r_int && d_dones && d_invalid && d_actor && d_h_ext && d_c_ext && d_h_int && d_c_int,
                 "srlx_seq_gather: an output pointer is NULL");
    SeqGatherArgs a{};
    a.B = B;
    a.L = (int)L;
    a.S = (int)S;
    a.A = (int)A;
    a.H = (int)H;
    a.frame_elems = frame_elems;
    a.frame_stride = frame_stride;
    a.frame_capacity = frame_capacity;
    a.seq_capacity = seq_capacity;
    a.record_stride = record_stride;
    a.slots = d_slots;
    a.ring = d_ring;
    a.records = d_records;
    a.states = d_states;
    a.actions = d_actions;
    a.r_ext = d_r_ext;
    a.r_int = d_r_int;
    a.dones = d_dones;
    a.invalid = d_invalid;
    a.actor = d_actor;
    a.h_ext = d_h_ext;
    a.c_ext = d_c_ext;
    a.h_int = d_h_int;
    a.c_int = d_c_int;
    const bool vec = frame_elems % 4 == 0 && frame_stride % 4 == 0 && aligned16(d_ring) && aligned16(d_states);  // one path per launch
    const i64 units = vec ? frame_elems / 4 : frame_elems;
    const dim3 grid((unsigned)(B * L + B), (unsigned)((units + kChunk - 1) / kChunk));
    if (vec)
        hipLaunchKernelGGL(k_seq_gather<float4>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_seq_gather<float>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    SRLX_HIP(hipGetLastError());
    return SRLX_OK;
}

}  // extern "C"
