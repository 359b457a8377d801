// digat_user_graph.inc — user graphs and category masks built on the device from category indices (digat_user_graph_build)
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

// =================================================================================================
// user-graph construction
// =================================================================================================
// The user graph of an impression is a pure function of its H category indices (DESIGN 3): slot t is valid iff 0 <= idx[t] < C,
// present[c] iff some valid slot has category c, and with U = H + C
//   A[i][j]       (i, j < H)  i == j, or both valid and idx[i] == idx[j]
//   A[i][H+c] = A[H+c][i]     slot i valid and idx[i] == c
//   A[H+a][H+b]               a == b, or present[a] and present[b]
//   mask[c] = present[c] (c < C), mask[C] = 0.
// All three blocks are one test on a per-NODE code byte: a valid history slot carries its category, a topic node of a present
// category carries 0x80 | category, every other node 0xFF (dead: self loop only).  Two live nodes are adjacent iff their categories
// are equal or both are topic nodes (C <= 127, so a category fits the low seven bits).
//
// One workgroup per graph (grid-stride).  The indices are staged in LDS as code bytes, present[] is counted there.  A graph is
// U * U bytes out for 8 H bytes in; its base g * U * U is odd for U = 67, so it is written as byte stores up to the first 16-byte
// boundary, naturally aligned 16-byte stores over the body, byte stores over the tail.  (Measured, DESIGN 8: the pair test per
// output byte, not HBM, bounds the kernel at 1.0 TB/s of writes.)
// entries[g] (set bytes of graph g) comes from the category counts n_c: U self loops, n_c (n_c - 1) + 2 n_c per category between
// its history slots and with its topic node, P (P - 1) between the P present topic nodes; one plain store by thread 0.
constexpr int UG_DEAD = 0xFF;

__device__ __forceinline__ unsigned ug_edge(int i, int j, unsigned ci, unsigned cj) {
    const unsigned live = (ci != UG_DEAD) & (cj != UG_DEAD);
    const unsigned same = ((ci ^ cj) & 0x7Fu) == 0u;
    const unsigned topics = (ci & cj) >> 7;
    return (i == j) | (live & (same | topics));
}

__global__ void __launch_bounds__(256) user_graph_build_kernel(const int64_t* cat_idx, const int64_t* rows, long G, int H, int C,
                                                               uint8_t* graph, uint8_t* cat_mask, int* entries) {
    __shared__ unsigned char code[DIGAT_MAX_NODES];       // node codes: [0, H) history slots, [H, H + C) topic nodes
    __shared__ int part[2][2];                            // per wave: sum of n_c (n_c + 1), number of present categories
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int U = H + C, uu = U * U;
    for (long g = blockIdx.x; g < G; g += gridDim.x) {
        const int64_t* idx = cat_idx + (rows ? rows[g] : g) * H;
        if (tid < H) {
            const int64_t v = idx[tid];
            code[tid] = (v >= 0 && v < C) ? (unsigned char)v : (unsigned char)UG_DEAD;
        }
        __syncthreads();
        int n = 0;
        if (tid < 128) {                                  // waves 0, 1: thread c counts the valid slots of category c (C <= 127)
            if (tid < C) {
                for (int t = 0; t < H; ++t) n += code[t] == tid;      // every lane reads the same byte: a broadcast
                cat_mask[g * (C + 1) + tid] = n > 0 ? 1 : 0;
            }
            if (tid == C) cat_mask[g * (C + 1) + C] = 0;
            int s = n * (n + 1), p = n > 0 ? 1 : 0;
            for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); p += __shfl_xor(p, o, 64); }
            if (lane == 0) { part[wave][0] = s; part[wave][1] = p; }
        }
        if (tid < C) code[H + tid] = n > 0 ? (unsigned char)(0x80 | tid) : (unsigned char)UG_DEAD;      // the counts read code[0, H) only
        __syncthreads();
        if (tid == 0 && entries) {
            const int P = part[0][1] + part[1][1];
            entries[g] = U + part[0][0] + part[1][0] + P * (P - 1);
        }
        uint8_t* out = graph + g * uu;
        const int head = min(uu, (int)((16 - ((uintptr_t)out & 15)) & 15));
        const int words = (uu - head) >> 4, tail = head + 16 * words;
        for (int w = tid; w < words; w += 256) {
            const int p0 = head + 16 * w;
            int i = p0 / U, j = p0 - i * U;
            unsigned ci = code[i];
            unsigned v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned word = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    word |= ug_edge(i, j, ci, code[j]) << (8 * k);
                    if (++j == U) { j = 0; i = min(i + 1, U - 1); ci = code[i]; }     // the clamp: after the graph's last byte
                }
                v[q] = word;
            }
            *reinterpret_cast<uint4*>(out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        if (tid < 32) {                                   // ragged ends: at most 15 bytes each
            const int p = tid < 16 ? tid : tail + (tid - 16);
            if (tid < 16 ? tid < head : p < uu) {
                const int i = p / U, j = p - i * U;
                out[p] = (uint8_t)ug_edge(i, j, code[i], code[j]);
            }
        }
        __syncthreads();                                  // code[] and part[] are rewritten by the next graph
    }
}

extern "C" int digat_user_graph_build(const int64_t* cat_idx, const int64_t* rows, long G, int H, int C, uint8_t* graph, uint8_t* cat_mask,
                                      int32_t* entries, void* stream) {
    if (!cat_idx || !graph || !cat_mask || G < 0 || H < 0 || C < 0) return DIGAT_ERR_ARG;
    if (H < 1 || C < 1 || H + C > DIGAT_MAX_NODES) return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    // 84 VGPRs: five workgroups of 256 threads are resident per CU, so 256 CUs x 5 fill the chip once (some store while others
    // stage their indices); the rest is the grid stride
    const long blocks = G < 1280 ? G : 1280;
    hipLaunchKernelGGL(user_graph_build_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, cat_idx, rows, G, H, C, graph,
                       cat_mask, entries);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}
