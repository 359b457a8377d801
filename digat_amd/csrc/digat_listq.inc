// digat_listq.inc — list quality: what a finished recommendation list looks like (the measure behind util.recommend_report: cosine
// diversity, category spread, overlap with the list before the second stage, catalogue exposure).  Included at the end of
// digat_kernels.hip, behind digat_mmr.inc (mmr_gram, MMR_MAX_M: sim(p, q) below is the Gram mmr_kernel selects on, so it has the bits
// of digat_dot_scores).
//
// listq_kernel, one workgroup (4 waves) per list:
//   threads 0 .. 127 take the list's ids (-1: beyond count[g] or outside [0, N): no element), each element's category into LDS and
//   its exposure[id] += 1 (an integer atomic, no return value: order-free and exact); threads 128 .. 255 take the base list's ids.
//   With vectors: mmr_gram, the [Mu, Mu] Gram of the gathered rows in LDS, Mu = count rounded up to 16 — the one product of
//   digat_mmr.inc, not a copy (what the sharing cost mmr_kernel — nothing it allocates — is in its header).  Without: no dynamic LDS at all.
//   Then all four waves reduce.  Waves 0 and 1: position tid against every position of the list — is an earlier element of its
//   category there (no: one more distinct category), how many elements share it (the wave's max) —, the compared entry an LDS
//   broadcast.  Waves 2 and 3: position tid - 128 against every base entry, likewise.  Every wave: the rows p = wave, wave + 4, ...
//   of the Gram's upper triangle, lanes along the row (q = lane and lane + 64: conflict-free), each lane summing its entries in
//   double and keeping their fmaxf in the order of p; then a butterfly over the wave (both partners add the same two numbers, so
//   every lane holds the same sum), the four waves' partials through LDS, and thread 0 adds them 0 + 1 + 2 + 3 and writes the list's
//   outputs.  The order of the sum depends on the list alone — not on the batch, not on timing; no float atomics.
//   A maximum of zero is written as +0.0 (max + 0.0f), so the bits do not depend on the order two zeros of either sign met in.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), 256 threads per workgroup; dynamic LDS 0
// without vectors, else mmr_kernel's 4 Mp max(Mp + 4, DOT_LD) bytes (2 304 B at k <= 16, 67 584 B at k = 128):
//   listq_kernel   VGPRs 46 + AGPRs 64 (the 2 x 8 accumulator tiles)   SGPRs 94   LDS 2656 B static   scratch 0   occupancy 4 waves / SIMD
//   (by registers; at k = 128 with vectors the 70 240 B of LDS allow two workgroups = 2 waves / SIMD)

struct ListqArgs {
    const int64_t* ids;
    const int32_t* count;
    long G;
    int k;
    long N;
    const float* vectors;
    int d;
    const int32_t* category;
    const int64_t* base_ids;
    const int32_t* base_count;
    int kb;
    int32_t* exposure;
    int32_t* elements;
    double* sim_sum;
    float* sim_max;
    int32_t* categories;
    int32_t* category_max;
    int32_t* overlap;
    int ld;                  // row stride of the Gram in LDS: k rounded up to 16, + 4
};

__global__ void __launch_bounds__(256) listq_kernel(const ListqArgs a) {
    extern __shared__ float4 listq_lds[];            // mmr_gram's: the staged rows, then the Gram [Mu][ld]
    __shared__ long long lid[MMR_MAX_M];             // vectors row of every list position, -1: not an element
    __shared__ long long lbase[MMR_MAX_M];           // the same of the base list
    __shared__ int lcat[MMR_MAX_M];
    __shared__ double wsum[4];
    __shared__ float wmax[4];
    __shared__ int wint[4][3];                       // per wave: elements, distinct categories | overlap, largest category
    float* const L = (float*)listq_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pos = tid & (MMR_MAX_M - 1);
    const long g = blockIdx.x;
    int cnt = a.count ? a.count[g] : a.k;
    cnt = cnt < 0 ? 0 : (cnt > a.k ? a.k : cnt);
    const int T = (cnt + 15) >> 4;                   // 16-row tiles of this list's Gram: <= 8, and 16 T <= ld - 4
    if (tid < MMR_MAX_M) {
        long long id = -1;
        if (tid < cnt) {
            id = (long long)a.ids[g * a.k + tid];
            if (id < 0 || id >= a.N) id = -1;
        }
        lid[tid] = id;
        lcat[tid] = id >= 0 && a.category ? a.category[id] : 0;
        if (id >= 0 && a.exposure) atomicAdd(a.exposure + id, 1);
    } else if (a.base_ids) {
        int bc = a.base_count ? a.base_count[g] : a.kb;
        bc = bc < 0 ? 0 : (bc > a.kb ? a.kb : bc);
        long long id = -1;
        if (pos < bc) {
            id = (long long)a.base_ids[g * a.kb + pos];
            if (id < 0 || id >= a.N) id = -1;
        }
        lbase[pos] = id;
    }
    __syncthreads();

    if (a.vectors) mmr_gram(L, lid, a.vectors, a.d, T, a.ld);

    // ---- the integer figures: waves 0 and 1 the categories of position tid, waves 2 and 3 the overlap of position tid - 128
    const long long id = lid[pos];
    const bool el = id >= 0;                         // then pos < cnt <= k
    int n_el = 0, n_a = 0, n_max = 0;
    if (wave < 2) {
        n_el = __popcll(__ballot(el));
        if (a.category) {
            const int c = lcat[pos];
            int same = 0;
            bool first = el;
            for (int q = 0; q < cnt; ++q) {
                const bool m = lid[q] >= 0 && lcat[q] == c;
                same += m;
                first = first && !(m && q < pos);
            }
            n_a = __popcll(__ballot(first));
            n_max = el ? same : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int other = __shfl_xor(n_max, o, 64);
                n_max = other > n_max ? other : n_max;
            }
        }
    } else if (a.base_ids) {
        bool hit = false;
        for (int q = 0; q < a.kb; ++q) hit = hit || lbase[q] == id;
        n_a = __popcll(__ballot(hit && el));          // a base entry that is no element holds -1: it meets no element's id
    }

    // ---- the upper triangle of the Gram: rows wave, wave + 4, ..., lanes along the row
    double sum = 0.0;
    float mx = -INFINITY;
    if (a.vectors) {
        const bool e0 = lid[lane] >= 0, e1 = lid[lane + 64] >= 0;
        for (int p = wave; p < cnt; p += 4) {
            if (lid[p] < 0) continue;                 // wave-uniform
            const float* const row = L + p * a.ld;
            if (e0 && lane > p) {
                const float s = row[lane];
                sum += (double)s;
                mx = fmaxf(mx, s);
            }
            if (e1 && lane + 64 > p) {
                const float s = row[lane + 64];
                sum += (double)s;
                mx = fmaxf(mx, s);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        }
    }
    if (lane == 0) {
        wsum[wave] = sum;
        wmax[wave] = mx;
        wint[wave][0] = n_el;
        wint[wave][1] = n_a;
        wint[wave][2] = n_max;
    }
    __syncthreads();
    if (tid != 0) return;
    a.elements[g] = wint[0][0] + wint[1][0];
    if (a.vectors) {
        a.sim_sum[g] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        a.sim_max[g] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])) + 0.0f;
    }
    if (a.category) {
        a.categories[g] = wint[0][1] + wint[1][1];
        a.category_max[g] = wint[0][2] > wint[1][2] ? wint[0][2] : wint[1][2];
    }
    if (a.base_ids) a.overlap[g] = wint[2][1] + wint[3][1];
}

extern "C" {

size_t digat_list_quality_workspace_bytes(int64_t lists, int k, int kb) {
    (void)lists; (void)k; (void)kb;
    return 0;                                        // the Gram never leaves LDS
}

int digat_list_quality(const int64_t* ids, const int32_t* count, int64_t G, int k, int64_t N, const float* vectors, int d,
                       const int32_t* category, const int64_t* base_ids, const int32_t* base_count, int kb, int32_t* exposure,
                       int32_t* out_elements, double* out_sim_sum, float* out_sim_max, int32_t* out_categories, int32_t* out_category_max,
                       int32_t* out_overlap, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;
    if (!ids || !out_elements || G < 0 || N < 0) return DIGAT_ERR_ARG;
    if ((vectors != nullptr) != (out_sim_sum != nullptr) || (vectors != nullptr) != (out_sim_max != nullptr)) return DIGAT_ERR_ARG;
    if ((category != nullptr) != (out_categories != nullptr) || (category != nullptr) != (out_category_max != nullptr)) return DIGAT_ERR_ARG;
    if ((base_ids != nullptr) != (out_overlap != nullptr) || (base_count && !base_ids) || (vectors && d < 1)) return DIGAT_ERR_ARG;
    if (k < 1 || k > MMR_MAX_M || (base_ids && (kb < 1 || kb > MMR_MAX_M)) || (vectors && d > (1 << 24)) || G > 0x7fffffffL)
        return DIGAT_ERR_SHAPE;
    if (G == 0) return DIGAT_OK;
    const int Mp = (k + 15) / 16 * 16;
    ListqArgs a{ids, count, (long)G, k, (long)N, vectors, d, category, base_ids, base_count, base_ids ? kb : 0, exposure, out_elements,
                out_sim_sum, out_sim_max, out_categories, out_category_max, out_overlap, Mp + 4};
    const size_t lds = vectors ? (size_t)Mp * (size_t)(Mp + 4 > DOT_LD ? Mp + 4 : DOT_LD) * sizeof(float) : 0;
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)listq_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DIGAT_ERR_LAUNCH;
    hipLaunchKernelGGL(listq_kernel, dim3((unsigned)G), dim3(256), lds, (hipStream_t)stream, a);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

}  // extern "C"
