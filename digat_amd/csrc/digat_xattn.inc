// digat_xattn.inc — Eq. 8 after the projections: score kernels (tile / small-graph), aggregation on the fp32 matrix cores, launch plan
// Included by digat_kernels.hip (one translation unit: hipcc --offload-arch=gfx950).

// =================================================================================================
// 2. Eq. 8 (a1/a2 after the projections): score kernel (VALU) + aggregation kernel (fp32 MFMA)
// =================================================================================================
// Score kernel.  One thread owns a 4x4 tile of (centre i, neighbour j) pairs and runs the whole sum
// over the d channels for it in registers (16 accumulators), so the scores need no cross-lane
// reduction.  P' = K3 + K1 (written by the projection GEMM's epilogue, the reference's left-to-right
// order) and Q stream through LDS in channel chunks by LDS-DMA (global_load_lds_dwordx4: no register
// round trip), a ring of XA_RING chunk images with two chunks in flight behind hand-counted
// s_waitcnt vmcnt and ONE raw s_barrier per chunk.  The DMA destination is lane-linear, so the
// permutation lives in the per-lane SOURCE address: image slot [pos][c4], pos = (node%4)*NT + node/4;
// with an odd chunk width (5 float4 at d = 400) the 16 lanes of a ds_read_b128 group hit distinct
// 16-B slots.  Slots of padding positions re-read a real node (finite, never used).
// Tiles whose 16 adjacency bytes are all zero are never computed: a per-workgroup list of the
// non-empty tiles is built from the adjacency image and threads are dealt tiles from that list, so
// whole waves drop out on sparse graphs (masked scores are replaced by -1e9 whatever their value).
// To make empty tiles common, the nodes of every row are first ORDERED by their first neighbour
// (stable rank sort in LDS): same-category history items and their topic node share that key, so the
// adjacency becomes block-diagonal.  The order only changes which node a tile slot holds (DMA source
// address, adjacency lookup); alpha is written in the caller's node order and its values do not depend
// on the order (each score is one thread's sequential channel sum).
// The kernel is VALU-bound (PMC: SQ_ACTIVE_INST_VALU ~ 96 % of the kernel, 4 cycles per wave64
// instruction), so the inner loop uses a.relu(x) = (a.x + a.|x|)/2: per (i,j,c) one v_add (x = p + q) and
// one v_fma with the free |x| source modifier instead of add + max + fma; the separable linear part
// a.P'_j + a.Q_i is accumulated once per node by the first 8*NT*RB threads.
// Scores go to LDS, one wave per (row, centre) does the masked softmax with shuffles and writes
// alpha [B,n,n]; [B,n,n,d] is never materialised.
struct ScoreArgs {
    const float* P;    // P' = r + P  (K3 + K1)
    const float* Q; const float* a; const uint8_t* A; float* alpha;
    float* s_out;      // optional [B,n,n]: scores before leaky_relu / mask on the edges (training)
    const uint8_t* live;   // optional [B,n]: 0 = dead node (see user_live_flags_kernel): its alpha row is not computed
    const int* qgroup;     // optional [B]: row b's Q lives at Q[qgroup[b]] (rows of one impression share the centre-side projection)
    const float* radd;     // optional [B,d] (small-graph kernel only): P holds K1 alone and K3 = radd[b] is added here
    const int64_t* bindex; // optional [B] (small-graph kernels, fused form): P, Q, agg_h, agg_x are TABLES and row b's graph is their
                           // row bindex[b] (per-news layer-0 tables read in place: no gathered copy); A, radd, the output stay per row
    const float* agg_h; const float* agg_x; float* agg_out;   // small-graph kernel only, all three or none: the wave also
                           // forms out_i = relu(sum_j alpha_ij h_j) + X_i (no alpha round trip, no aggregation launch)
    int B, n, d, d4;
    int NT, SN, CC4, nchunks, RB;
    int img_slots;     // float4 slots of one operand image of one chunk = RB * 4*NT * CC4
    int ring_slots;    // slots of one ring buffer: both operands, padded to a multiple of 64
    int ninstr;        // DMA wave-instructions per chunk = ring_slots / 64
    int am_off;        // byte offset of the adjacency BIT rows in LDS: [RB*n][NW] words, NW = ceil(n/32)
    int a_off;         // byte offset of a (d floats) in LDS
    int tl_off;        // byte offset of the non-empty-tile list (ints) + per-wave counters
    int ld_off;        // byte offset of the per-node linear terms a.P'_j, a.Q_i (2 * RB * 4*NT floats)
    int pm_off;        // byte offset of the node permutation: keys [RB*n] ints, then node_of [RB*n] ints
    const int* skip_if;    // optional device int: the launch returns at once when *skip_if != 0 (the sparse kernel does this batch)
    // training (round 6): the attention dropout is applied where alpha is produced (amask != NULL): keep bytes [B,n,n] by the
    // counter hash of (drop_seed, flat index), alpha itself stays undropped for the backward, adrop (tile kernel; the small-graph
    // kernel aggregates from registers) receives drop_p(alpha)
    uint8_t* amask; float* adrop; float drop_p; unsigned drop_seed;
};
// XA_RING (chunk images in the LDS ring), XA_KMAX (DMA wave-instructions a wave issues per chunk): digat_xattn_plan.h

// the geometry of a tile plan as kernel arguments; the caller adds its pointers by name
static ScoreArgs score_args(const XattnTile& t) {
    ScoreArgs g = {};
    g.B = t.B; g.n = t.n; g.d = t.d; g.d4 = t.d4;
    g.NT = t.NT; g.SN = t.SN; g.CC4 = t.CC4; g.nchunks = t.nchunks; g.RB = t.RB;
    g.img_slots = t.img_slots; g.ring_slots = t.ring_slots; g.ninstr = t.ninstr;
    g.am_off = t.am_off; g.a_off = t.a_off; g.tl_off = t.tl_off; g.ld_off = t.ld_off; g.pm_off = t.pm_off;
    return g;
}
// A route's width class as a template parameter: f(std::integral_constant<int, U>) for U = 1, 2, and 4 where MAXU = 4 (the kernels
// that keep several centres per wave, and the entry-wise backward, have no instantiation at four pieces per lane)
template <int MAXU, class F>
static inline void eq8_by_width(int U, F&& f) {
    switch (U) {
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 4: if constexpr (MAXU >= 4) f(std::integral_constant<int, 4>()); break;
    }
}


__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(5, 8))) xattn_score_kernel(const ScoreArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (g.skip_if && *g.skip_if != 0) return;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = nthreads >> 6;
    const int b0 = blockIdx.x * g.RB;
    const int rows_here = min(g.RB, g.B - b0);
    const int n = g.n, NT = g.NT, CC4 = g.CC4, SN = g.SN, d4 = g.d4;

    float4* ring = reinterpret_cast<float4*>(smem);        // [XA_RING][ring_slots]: P' image, then Q image
    float* Ss = reinterpret_cast<float*>(smem);            // [RB][n][SN], aliases the ring after the chunk loop
    unsigned* Ab = reinterpret_cast<unsigned*>(smem + g.am_off);   // adjacency bit rows [RB*n][NW]
    const int NW = (n + 31) >> 5;
    float4* a_lds = reinterpret_cast<float4*>(smem + g.a_off);
    int* tl = reinterpret_cast<int*>(smem + g.tl_off);     // [RB*NT*NT] tile list, then [16] wave counts
    int* wcnt = tl + g.RB * NT * NT;
    float* lin = reinterpret_cast<float*>(smem + g.ld_off);   // [2][RB][4*NT]: a.P'_node, a.Q_node by image position
    const unsigned ring_lds = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

    // ---- phase 0: the adjacency bytes pass through the (still idle) ring area with wide loads and are
    // condensed to bit rows; the score vector a goes to LDS
    {
        // 16-byte loads from the enclosing aligned window
        const uint8_t* src = g.A + (long)b0 * n * n;
        const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 15);
        const uint4* src16 = reinterpret_cast<const uint4*>(src - mis);
        const int nvec = (rows_here * n * n + mis + 15) >> 4;
        uint4* dst16 = reinterpret_cast<uint4*>(smem);
        for (int i = tid; i < nvec; i += nthreads) dst16[i] = src16[i];
        const float4* a4 = reinterpret_cast<const float4*>(g.a);
        for (int i = tid; i < d4; i += nthreads) a_lds[i] = a4[i];
        __syncthreads();
        const uint8_t* bytes = smem + mis;
        for (int e = tid; e < rows_here * n * NW; e += nthreads) {
            const int row = e / NW, w = e - row * NW;
            unsigned bits = 0;
            const uint8_t* br = bytes + row * n + w * 32;
            const int lim = min(32, n - w * 32);
            for (int k = 0; k < lim; ++k) bits |= (br[k] != 0 ? 1u : 0u) << k;
            if (g.live && !g.live[(long)b0 * n + row]) bits = 0;      // a dead node's row: no pair of it is ever needed
            Ab[e] = bits;
        }
    }
    __syncthreads();
    auto edge = [&](int rb, int i, int j) -> bool { return (Ab[(rb * n + i) * NW + (j >> 5)] >> (j & 31)) & 1u; };

    // ---- node order: stable sort of each row's nodes by their first neighbour (block-diagonalises the
    // category structure of user graphs; any order is legal)
    int* keys = reinterpret_cast<int*>(smem + g.pm_off);       // [RB*n]
    int* node_of = keys + g.RB * n;                            // [RB*n]: node held by sorted slot sig
    for (int e = tid; e < rows_here * n; e += nthreads) {
        const int rb = e / n, i = e - rb * n;
        int key = g.live ? n + i : i;        // rows without any bit (dead nodes, when a list is given) go last, together
        for (int w = 0; w < NW; ++w) {
            const unsigned bits = Ab[e * NW + w];
            if (bits) { key = w * 32 + __ffs(bits) - 1; break; }
        }
        keys[e] = key;
    }
    __syncthreads();
    for (int e = tid; e < rows_here * n; e += nthreads) {
        const int rb = e / n, i = e - rb * n;
        const int key = keys[e];
        int rank = 0;
        for (int k = 0; k < n; ++k) {
            const int kk = keys[rb * n + k];
            rank += (kk < key) || (kk == key && k < i);
        }
        node_of[rb * n + rank] = i;
    }
    __syncthreads();

    // ---- this wave's DMA pieces: instruction q = wave + nwaves*k covers image slots [64q, 64q+64)
    const float* Pblk = g.P + (long)b0 * n * g.d;
    const float* Qblk = g.qgroup ? g.Q : g.Q + (long)b0 * n * g.d;      // grouped: offsets below are absolute rows of Q
    int src_off[XA_KMAX];        // float offset of this lane's source at chunk 0; bit 31: Q operand
    int kw = 0;                  // wave-uniform: instructions this wave issues per chunk
#pragma unroll
    for (int k = 0; k < XA_KMAX; ++k) {
        const int q = wave + nwaves * k;
        src_off[k] = 0;
        if (q < g.ninstr) {
            kw = k + 1;
            int slot = q * 64 + lane;
            if (slot >= 2 * g.img_slots) slot = 2 * g.img_slots - 1;           // padding lanes re-read the last slot
            const int op = slot >= g.img_slots;
            const int e = slot - op * g.img_slots;
            const int per_row = 4 * NT * CC4;
            int rb = e / per_row;
            const int rem = e - rb * per_row;
            const int pos = rem / CC4, c4 = rem - pos * CC4;
            int sig = (pos % NT) * 4 + pos / NT;                               // sorted slot held by this image position
            if (sig >= n) sig = n - 1;                                         // padding positions: any real node
            if (rb >= rows_here) rb = rows_here - 1;
            int node = node_of[rb * n + sig];
            if (g.live && !g.live[(long)(b0 + rb) * n + node]) node = node_of[rb * n];      // dead: re-read the first (live) node, never used
            const int brow = (op && g.qgroup) ? g.qgroup[b0 + rb] : rb;
            src_off[k] = ((brow * n + node) * g.d + c4 * 4) | (op << 31);
        }
    }
    auto issue = [&](int ch, int buf) {
#pragma unroll
        for (int k = 0; k < XA_KMAX; ++k) {
            if (k < kw) {
                const int q = wave + nwaves * k;
                const float* base = (src_off[k] < 0) ? Qblk : Pblk;
                lds_dma16(base + (src_off[k] & 0x7fffffff) + ch * CC4 * 4,
                          ring_lds + (unsigned)((buf * g.ring_slots + q * 64) * 16));
            }
        }
    };
    issue(0, 0);
    if (g.nchunks > 1) issue(1, 1);

    // ---- non-empty tiles -> compact list (order = tile id, deterministic)
    const int tiles = NT * NT;
    int my_tile = -1;
    {
        const int t = tid;
        bool flag = false;
        if (t < rows_here * tiles) {
            const int rb = t / tiles, tt = t - rb * tiles;
            const int ti = tt / NT, tj = tt - ti * NT;
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int si = 4 * ti + ii;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int sj = 4 * tj + jj;
                    if (si < n && sj < n && edge(rb, node_of[rb * n + si], node_of[rb * n + sj])) flag = true;
                }
            }
        }
        const unsigned long long mask = __ballot(flag);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < nwaves; ++w) {
            const int c = wcnt[w];
            if (w < wave) base += c;
            total += c;
        }
        if (flag) tl[base + before] = t;
        __syncthreads();
        if (tid < total) my_tile = tl[tid];
    }
    const bool active = my_tile >= 0;
    const int rb_t = active ? my_tile / tiles : 0;
    const int tt = active ? my_tile - rb_t * tiles : 0;
    const int ti = tt / NT, tj = tt - ti * NT;

    // ---- phase 1: scores
    float acc[4][4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.f;

    const int lin_rows = 2 * g.RB * 4 * NT;       // image rows: P' rows of every row-block, then Q rows
    float ldot = 0.f;                               // thread tid < lin_rows: a . (image row tid)
    for (int ch = 0; ch < g.nchunks; ++ch) {
        // chunk ch has landed once at most the newer chunk's pieces of THIS wave are outstanding ...
        wait_vmcnt(ch + 1 < g.nchunks ? kw : 0);
        // ... and every wave has said so: the barrier publishes chunk ch and retires chunk ch-1's readers
        __builtin_amdgcn_s_barrier();
        if (ch + 2 < g.nchunks) issue(ch + 2, (ch + 2) % XA_RING);      // into the image read in iteration ch-1
        if (active) {
            const float4* Pb = ring + (ch % XA_RING) * g.ring_slots + rb_t * 4 * NT * CC4;
            const float4* Qb = Pb + g.img_slots;
            const float4* av = a_lds + ch * CC4;
            for (int c4 = 0; c4 < CC4; ++c4) {
                const float4 a4 = av[c4];                     // same address in every lane: LDS broadcast
                float4 p[4], q[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) p[jj] = Pb[(jj * NT + tj) * CC4 + c4];
#pragma unroll
                for (int ii = 0; ii < 4; ++ii) q[ii] = Qb[(ii * NT + ti) * CC4 + c4];
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float sc = acc[ii][jj];          // accumulates sum_c a_c |x_c|
                        sc = fmaf(a4.x, fabsf(p[jj].x + q[ii].x), sc);
                        sc = fmaf(a4.y, fabsf(p[jj].y + q[ii].y), sc);
                        sc = fmaf(a4.z, fabsf(p[jj].z + q[ii].z), sc);
                        sc = fmaf(a4.w, fabsf(p[jj].w + q[ii].w), sc);
                        acc[ii][jj] = sc;
                    }
            }
        }
        if (tid < lin_rows) {   // the separable part sum_c a_c (P'_jc + Q_ic), once per node
            const float4* row = ring + (ch % XA_RING) * g.ring_slots + tid * CC4;      // P' rows then Q rows: contiguous
            const float4* av = a_lds + ch * CC4;
            for (int c4 = 0; c4 < CC4; ++c4) {
                const float4 v = row[c4], a4 = av[c4];
                ldot = fmaf(a4.w, v.w, fmaf(a4.z, v.z, fmaf(a4.y, v.y, fmaf(a4.x, v.x, ldot))));
            }
        }
    }
    if (tid < lin_rows) lin[tid] = ldot;
    __syncthreads();            // every wave is done with the ring: Ss may alias it

    // ---- phase 2a: every score starts masked (-1e9, not -inf)
    for (int i = tid; i < rows_here * n * SN; i += nthreads) Ss[i] = -1e9f;
    __syncthreads();
    // leaky_relu(0.2) of the computed scores where the adjacency has an edge
    if (active) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            if (4 * ti + ii >= n) continue;
            const int i = node_of[rb_t * n + 4 * ti + ii];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                if (4 * tj + jj >= n) continue;
                const int j = node_of[rb_t * n + 4 * tj + jj];
                if (edge(rb_t, i, j)) {
                    // a.relu(x) = (a.x + a.|x|) / 2
                    const float e = 0.5f * (acc[ii][jj] + (lin[rb_t * 4 * NT + jj * NT + tj]
                                                          + lin[(g.RB + rb_t) * 4 * NT + ii * NT + ti]));
                    if (g.s_out) g.s_out[((long)(b0 + rb_t) * n + i) * n + j] = e;
                    Ss[(rb_t * n + i) * SN + j] = e > 0.f ? e : 0.2f * e;
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 2b: softmax over the neighbours j, one wave per (row, centre i); a row without any
    // edge is all -1e9 and comes out uniform, as in the reference
    for (int rho = wave; rho < rows_here * n; rho += nwaves) {
        if (g.live && !g.live[(long)b0 * n + rho]) continue;           // dead centre: its alpha row keeps its (finite) old values
        const float* srow = Ss + (long)rho * SN;
        const float v0 = lane < n ? srow[lane] : -INFINITY;
        const float v1 = lane + 64 < n ? srow[lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(v0, v1));
        const float e0 = lane < n ? expf(v0 - m) : 0.f;
        const float e1 = lane + 64 < n ? expf(v1 - m) : 0.f;
        const float inv = wave_sum(e0 + e1);
        float* arow = g.alpha + ((long)b0 * n + rho) * n;
        if (lane < n) arow[lane] = e0 / inv;
        if (lane + 64 < n) arow[lane + 64] = e1 / inv;
        if (g.amask) {                                                  // wave-uniform
            const long e = ((long)b0 * n + rho) * n;
            const float scale = 1.f / (1.f - g.drop_p);
            const unsigned thr = drop_threshold(g.drop_p);
            if (lane < n) {
                const bool keep = drop_keep(g.drop_seed, e + lane, thr);
                g.amask[e + lane] = keep;
                g.adrop[e + lane] = keep ? (e0 / inv) * scale : 0.f;
            }
            if (lane + 64 < n) {
                const bool keep = drop_keep(g.drop_seed, e + lane + 64, thr);
                g.amask[e + lane + 64] = keep;
                g.adrop[e + lane + 64] = keep ? (e1 / inv) * scale : 0.f;
            }
        }
    }
}

// Score kernel for SMALL graphs (n <= 16: the news graph, N = 10 by default).  The tile kernel above would
// keep 72 of 256 threads busy there and pay a barrier + DMA round trip per 20-channel chunk; with so little
// arithmetic the job is a latency problem.  Here one WAVE owns one (row, centre i): the lanes span the channels
// (float4 each, coalesced), Q_i and a stay in registers, every neighbour's P'_j streams through once, the
// per-pair channel sum is a wave reduction, lane j keeps score j, and the masked softmax is the same
// shuffle code as above.  No LDS, no barrier; B*n waves (10 240 for the default batch).
template <int U>   // float4 pieces per lane: d <= 256 * U
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) xattn_score_small_kernel(const ScoreArgs g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rho = (long)blockIdx.x * 4 + wave;
    const int n = g.n, d4 = g.d4;
    if (rho >= (long)g.B * n) return;
    const long b = rho / n;
    const long bs = g.bindex ? (long)g.bindex[b] : b;        // source graph of the operand tables
    const float4* a4 = reinterpret_cast<const float4*>(g.a);
    const float4* Qi = reinterpret_cast<const float4*>(g.Q) + (g.qgroup ? (long)g.qgroup[b] * n + (rho - b * n) : bs * n + (rho - b * n)) * d4;
    const float4* Pb = reinterpret_cast<const float4*>(g.P) + bs * n * d4;
    // straight-line loads (padding lanes re-read the last piece and get a = 0): with a branch per load the compiler
    // sinks every request next to its use and the wave pays one global round trip per row
    float4 q[U], av[U];
    const float4* r4 = g.radd ? reinterpret_cast<const float4*>(g.radd) + b * d4 : a4;      // any valid address when unused
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        const float4 qv = Qi[c4], rv = r4[c4], aa = a4[c4];
        // K3 not yet in P (the projection ran before the other graph's context was known): x = K1_j + (K2_i + K3)
        q[u] = g.radd ? f4_add(qv, rv) : qv;
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();          // a = 0 on the padding channels: they add nothing
    }
    const bool edge = g.A[rho * n + min(lane, n - 1)] != 0 && lane < n;
    float mine = 0.f;
    auto pair_sum = [&](const float4 (&p)[U]) -> float {
        float part = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            part = fmaf(av[u].x, fmaxf(p[u].x + q[u].x, 0.f), part);
            part = fmaf(av[u].y, fmaxf(p[u].y + q[u].y, 0.f), part);
            part = fmaf(av[u].z, fmaxf(p[u].z + q[u].z, 0.f), part);
            part = fmaf(av[u].w, fmaxf(p[u].w + q[u].w, 0.f), part);
        }
        return wave_sum(part);
    };
    // SG neighbours' rows are requested before the first is used: the kernel is a chain of global round trips per wave
    // (there are only B*n waves), so the fewer dependent ones the better; slots past n repeat the last row (unused)
    constexpr int SG = 5;
    for (int j0 = 0; j0 < n; j0 += SG) {
        float4 p[SG][U];
#pragma unroll
        for (int t = 0; t < SG; ++t)
#pragma unroll
            for (int u = 0; u < U; ++u) p[t][u] = Pb[(long)min(j0 + t, n - 1) * d4 + min(lane + 64 * u, d4 - 1)];
#pragma unroll
        for (int t = 0; t < SG; ++t) {
            const float st = pair_sum(p[t]);                  // slots past n: a repeated row, never selected (lane < n <= j0 + t)
            mine = (lane == j0 + t && j0 + t < n) ? st : mine;
        }
    }
    if (edge && g.s_out) g.s_out[rho * n + lane] = mine;
    const float lk = mine > 0.f ? mine : 0.2f * mine;
    const float v0 = lane < n ? (edge ? lk : -1e9f) : -INFINITY;     // masked: -1e9, not -inf (a row without edges -> uniform)
    const float m = wave_max(v0);
    const float e0 = lane < n ? expf(v0 - m) : 0.f;
    const float inv = wave_sum(e0);
    float al = e0 / inv;
    if (g.s_out || !g.agg_out) {                 // training keeps alpha (before its dropout) for the backward
        if (lane < n) g.alpha[rho * n + lane] = al;
    }
    if (g.amask) {                               // attention dropout in place (training): keep bytes out, the aggregation below uses drop_p(alpha)
        const bool keep = lane < n && drop_keep(g.drop_seed, rho * n + lane, drop_threshold(g.drop_p));
        if (lane < n) g.amask[rho * n + lane] = keep;
        al = keep ? al * (1.f / (1.f - g.drop_p)) : 0.f;
        if (g.adrop && lane < n) g.adrop[rho * n + lane] = al;
    }
    if (!g.agg_out) return;
    // fused aggregation: lane j holds alpha_ij; the sum over the neighbours runs in ascending j (one fma chain per channel)
    const float4* Hb = reinterpret_cast<const float4*>(g.agg_h) + bs * n * d4;
    float4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f4_zero();
    for (int j0 = 0; j0 < n; j0 += SG) {
        float4 hv[SG][U];
#pragma unroll
        for (int t = 0; t < SG; ++t)
#pragma unroll
            for (int u = 0; u < U; ++u) hv[t][u] = Hb[(long)min(j0 + t, n - 1) * d4 + min(lane + 64 * u, d4 - 1)];
#pragma unroll
        for (int t = 0; t < SG; ++t) {
            const float a = j0 + t < n ? lane_bcast(al, min(j0 + t, 63)) : 0.f;        // slots past n: weight 0
            // a weight of exactly zero — a masked pair: exp(-1e9 - max) = 0 — is skipped by a wave-uniform branch, never multiplied:
            // the h row of a dead node (news_live_flags_kernel: neither projected nor written) may hold anything, and 0 x NaN = NaN
            if (a == 0.f) continue;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc[u].x = fmaf(a, hv[t][u].x, acc[u].x); acc[u].y = fmaf(a, hv[t][u].y, acc[u].y);
                acc[u].z = fmaf(a, hv[t][u].z, acc[u].z); acc[u].w = fmaf(a, hv[t][u].w, acc[u].w);
            }
        }
    }
    const float4* Xi = reinterpret_cast<const float4*>(g.agg_x) + (bs * n + (rho - b * n)) * d4;
    float4* Oi = reinterpret_cast<float4*>(g.agg_out) + rho * d4;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = lane + 64 * u;
        if (c4 < d4) {
            const float4 x = Xi[c4];
            Oi[c4] = make_float4(fmaxf(acc[u].x, 0.f) + x.x, fmaxf(acc[u].y, 0.f) + x.y,
                                 fmaxf(acc[u].z, 0.f) + x.z, fmaxf(acc[u].w, 0.f) + x.w);
        }
    }
}

// The same function with the GRAPH IN LDS (round 3).  The wave-per-centre kernel above lets every centre's wave fetch its
// neighbours' P' and h rows for itself: n waves x (2 n + 2) rows per graph, 153 MB of fabric traffic per launch for 84 MB of
// distinct bytes at N = 10.  Here one workgroup of four waves owns one graph: P' and h of its n <= 16 nodes (2 n d floats: 32 KB
// at N = 10, d = 400) go global -> LDS once by LDS-DMA (1 KB pieces, no registers), Q_i (+ K3), X_i and the adjacency row of the
// wave's centres (i = wave, wave + 4, ...) are requested at the same time into registers, then one wait + one barrier, and the
// scores, the masked softmax and the aggregation run from LDS with conflict-free ds_read_b128 (lanes span the channels).  Only
// the adjacency row's set bits are visited: a masked pair is exp(-1e9 - max) = 0 exactly and fma(0, h, acc) = acc, so the
// results are BIT-IDENTICAL to xattn_score_small_kernel's (same lane -> channel map, same fma and reduction order, neighbours
// ascending); a row without any edge is uniform over all n nodes, as there.  Needs the fused form (agg_*), no qgroup / s_out.
template <int U>   // float4 pieces per lane: d <= 256 * U
__global__ void __launch_bounds__(256) xattn_small_lds_kernel(const ScoreArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int MAXC = 4;                    // centres per wave: n <= 16
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = g.n, d4 = g.d4;
    const long b = blockIdx.x;
    const long bs = g.bindex ? (long)g.bindex[b] : b;         // source graph of the operand tables
    const int slots = n * d4;                  // float4 slots of one image (P' or h of this graph)
    const int pieces = (slots + 63) >> 6;      // 1 KB DMA pieces per image
    const float4* Ps = reinterpret_cast<const float4*>(smem);
    const float4* Hs = Ps + pieces * 64;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const float4* Pg = reinterpret_cast<const float4*>(g.P) + bs * slots;
    const float4* Hg = reinterpret_cast<const float4*>(g.agg_h) + bs * slots;
    for (int q = wave; q < 2 * pieces; q += 4) {             // lanes past the image re-read its last slot into the padding
        const int img = q >= pieces ? 1 : 0, qq = q - img * pieces;
        const int sl = min(qq * 64 + lane, slots - 1);
        lds_dma16(reinterpret_cast<const float*>((img ? Hg : Pg) + sl), lds0 + (unsigned)((q * 64) * 16));
    }
    const float4* a4 = reinterpret_cast<const float4*>(g.a);
    const float4* r4 = g.radd ? reinterpret_cast<const float4*>(g.radd) + b * d4 : a4;      // any valid address when unused
    float4 av[U], rv[U], q[MAXC][U], xin[MAXC][U];
    uint8_t ab[MAXC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        const float4 aa = a4[c4];
        rv[u] = r4[c4];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();          // a = 0 on the padding channels: they add nothing
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = min(wave + 4 * c, n - 1);               // centres past n: a repeated row, never used
        const long rho = b * n + i, rsrc = bs * n + i;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c4 = min(lane + 64 * u, d4 - 1);
            q[c][u] = (reinterpret_cast<const float4*>(g.Q) + rsrc * d4)[c4];
            xin[c][u] = (reinterpret_cast<const float4*>(g.agg_x) + rsrc * d4)[c4];
        }
        ab[c] = g.A[rho * n + min(lane, n - 1)];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int i = wave + 4 * c;
        if (i >= n) break;                                    // wave-uniform
        const long rho = b * n + i;
        float4 qc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) qc[u] = g.radd ? f4_add(q[c][u], rv[u]) : q[c][u];      // x = K1_j + (K2_i + K3)
        const bool edge = ab[c] != 0 && lane < n;
        unsigned m = (unsigned)__ballot(edge);
        float mine = 0.f;
        for (unsigned mm = m; mm; mm &= mm - 1u) {
            const int j = __builtin_ctz(mm);
            float part = 0.f;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4 p = Ps[j * d4 + min(lane + 64 * u, d4 - 1)];
                part = fmaf(av[u].x, fmaxf(p.x + qc[u].x, 0.f), part);
                part = fmaf(av[u].y, fmaxf(p.y + qc[u].y, 0.f), part);
                part = fmaf(av[u].z, fmaxf(p.z + qc[u].z, 0.f), part);
                part = fmaf(av[u].w, fmaxf(p.w + qc[u].w, 0.f), part);
            }
            const float st = wave_sum(part);
            mine = lane == j ? st : mine;
        }
        const float lk = mine > 0.f ? mine : 0.2f * mine;
        const float v0 = lane < n ? (edge ? lk : -1e9f) : -INFINITY;     // masked: -1e9, not -inf (a row without edges -> uniform)
        const float mx = wave_max(v0);
        const float e0 = lane < n ? expf(v0 - mx) : 0.f;
        const float inv = wave_sum(e0);
        const float al = e0 / inv;
        if (m == 0u) m = (1u << n) - 1u;                      // no edge at all: every node with weight 1 / n
        float4 acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = f4_zero();
        for (unsigned mm = m; mm; mm &= mm - 1u) {
            const int j = __builtin_ctz(mm);
            const float w = lane_bcast(al, j);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4 hv = Hs[j * d4 + min(lane + 64 * u, d4 - 1)];
                acc[u].x = fmaf(w, hv.x, acc[u].x); acc[u].y = fmaf(w, hv.y, acc[u].y);
                acc[u].z = fmaf(w, hv.z, acc[u].z); acc[u].w = fmaf(w, hv.w, acc[u].w);
            }
        }
        float4* Oi = reinterpret_cast<float4*>(g.agg_out) + rho * d4;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c4 = lane + 64 * u;
            if (c4 < d4) {
                const float4 x = xin[c][u];
                Oi[c4] = make_float4(fmaxf(acc[u].x, 0.f) + x.x, fmaxf(acc[u].y, 0.f) + x.y,
                                     fmaxf(acc[u].z, 0.f) + x.z, fmaxf(acc[u].w, 0.f) + x.w);
            }
        }
    }
}

// Eq. 8 on SPARSE graphs, score + softmax + aggregation in one launch (the MIND user graph: 67 nodes, ~4 edges per
// node — identity, the node's topic, same-category history items, topic-topic).  The tile kernel above streams all
// 2 x 68 x d projections of a row through LDS and the MFMA aggregation multiplies a dense [n,n] alpha whatever the
// adjacency holds; with so few edges both are launch-cadence and bandwidth for nothing.  Here one WAVE owns one centre
// (b, i): the adjacency row becomes two 64-bit ballots, and only the set bits are visited — once for the scores
// (P'_j streams from L2: the rows of one graph are shared by its centres), once, after the masked softmax in
// registers (lane j keeps alpha_ij), for sum_j alpha_ij h_j.  Lanes span the channels (float4 pieces), a, Q_i (and
// K3_b when the projection ran before K3 was known) stay in registers, four neighbours are in flight.  Masked
// pairs contribute exp(-1e9 - max) = 0 exactly, so leaving them out changes nothing; a centre without ANY entry is all
// -1e9 in the reference, i.e. uniform over every node (E5), and is computed as that.  alpha is never written.
// Whether a batch is sparse is decided on the device (sparse_decide_kernel: total entries of the adjacency); this
// kernel and the dense pair (tile score + MFMA aggregation) are both launched and the one that is not wanted returns
// at its first instruction.
struct SparseArgs {
    const float* P; const float* Q; const float* h; const float* X; const float* a; const uint8_t* A; float* out;
    const float* radd;       // optional [B,d]: P holds K1 alone and P'_j = K3_b + K1_j is formed here (the order of the GEMM epilogue)
    const int* group;        // optional [B]: P / Q / h of row b live at row group[b] (rows of one impression share them)
    const uint8_t* live;     // optional [B,n]: dead centres are skipped (neither read nor written)
    const int* run_if;       // optional device int: run iff *run_if != 0
    int B, n, d4;
    int xgroup;                                  // with group: X too is given once per group ([G,n,d]) and read through it
    const uint8_t* fill_flags; float* fill_out;  // optional: centres with fill_flags[b*n+i] == 0 also write X_i to fill_out's row
                                                 // (see the caller: a buffer whose dead rows would otherwise stay uninitialised)
    const int* rowidx; const int* nrows_dev;     // optional, with live: the live centres b*n+i in ascending order and their count
                                                 // (the list of the projection GEMM): waves beyond it return without a load
    int G;                                       // with group: the number of groups (profiling: distinct rows behind the index)
    unsigned long long* exec_rows;               // profiling, with rowidx: the launch adds *nrows_dev x exec_unit BYTES here (see launch_sparse)
    int pq16;                                    // wave-per-centre kernel only: 1 = P and Q are bf16 rows, 2 = block-scaled e4m3 rows
    int centre_limit;                            // > 0: centres i >= centre_limit are not computed (nobody reads their rows:
                                                 // the last layer's topic nodes — the user context pools the history rows only)
    int xcd_group;                               // > 0: workgroups are dealt to the 8 XCDs in runs of xcd_group (see the kernel)
    long ld8;                                    // pq16 == 2: bytes between rows ([d codes | d / 80 fp32 scales | pad]: the GEMM's fp8 segments)
    const unsigned* twin; const int* twlist; const int* twcount;   // optional, with rowidx: centres with EQUAL adjacency rows served together
                                                 // (user_live_flags_kernel's twin words [B n], the list of the leading centres, their count)
    unsigned exec_unit;                          // with exec_rows: algorithmic bytes per live centre of the list (0: a counting kernel prices the launch)
    int prof_part;                               // profiling: 0 = the part follows from the arguments (sparse_part), else XPART_* + 1 (the news graph's row-list launches)
    // training (xattn_sparse_kernel<., 0, false, true>; round 6): what the backward needs leaves the wave — the centre's alpha row
    // [n] BEFORE its dropout, the scores before leaky_relu on the adjacency's entries — and the attention dropout is applied in
    // place (t_amask != NULL: keep bytes [n] by the counter hash of (t_seed, rho n + j); the aggregation uses drop_p(alpha))
    float* t_alpha; float* t_spre; uint8_t* t_amask; float t_p; unsigned t_seed;
#ifdef DIGAT_SPARSE_TIMERS
    unsigned long long* timers;                  // experiment builds only: [9] phase cycle sums of sampled waves
#endif
};

#ifdef DIGAT_SPARSE_TIMERS
// experiment builds only (tools/exp): a sampled wave drains its queues at each phase boundary and adds the cycles to timers[k]
#define SP_T0() unsigned long long sp_last = __builtin_amdgcn_s_memtime(); const bool sp_on = g.timers && (blockIdx.x & 15) == 0
#define SP_T(k) do { if (sp_on) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t__ = __builtin_amdgcn_s_memtime(); \
                     if (lane == 0) atomicAdd(g.timers + (k), t__ - sp_last); sp_last = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define SP_T0() do {} while (0)
#define SP_T(k) do {} while (0)
#endif

#ifndef DIGAT_SPARSE_NBR
#define DIGAT_SPARSE_NBR 4
#endif
// a . relu(p + q) over the 8 channels of one 16-byte piece of bf16 rows (a in fp32: two float4), added to `part`
__device__ __forceinline__ float score8_bf16(const uint4 p, const uint4 q, const float4 a0, const float4 a1, float part) {
    const unsigned pw[4] = {p.x, p.y, p.z, p.w}, qw[4] = {q.x, q.y, q.z, q.w};
    const float aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float p0 = __builtin_bit_cast(float, pw[k] << 16), p1 = __builtin_bit_cast(float, pw[k] & 0xffff0000u);
        const float q0 = __builtin_bit_cast(float, qw[k] << 16), q1 = __builtin_bit_cast(float, qw[k] & 0xffff0000u);
        part = fmaf(aw[2 * k], fmaxf(p0 + q0, 0.f), part);
        part = fmaf(aw[2 * k + 1], fmaxf(p1 + q1, 0.f), part);
    }
    return part;
}

// a . relu(p s_p + q) over the 8 channels of one 8-byte piece of an e4m3 row: the neighbour's codes are converted two at a time
// (v_cvt_pk_f32_fp8) and rescaled by the fma that adds the centre's Q piece (already in fp32: converted and rescaled once per centre)
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float score8_fp8(const uint2 p, const float sp, const float (&qf)[8], const float4 a0, const float4 a1, float part) {
    const f2v p01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.x, false), p23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.x, true);
    const f2v p45 = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.y, false), p67 = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.y, true);
    part = fmaf(a0.x, fmaxf(fmaf(p01[0], sp, qf[0]), 0.f), part);
    part = fmaf(a0.y, fmaxf(fmaf(p01[1], sp, qf[1]), 0.f), part);
    part = fmaf(a0.z, fmaxf(fmaf(p23[0], sp, qf[2]), 0.f), part);
    part = fmaf(a0.w, fmaxf(fmaf(p23[1], sp, qf[3]), 0.f), part);
    part = fmaf(a1.x, fmaxf(fmaf(p45[0], sp, qf[4]), 0.f), part);
    part = fmaf(a1.y, fmaxf(fmaf(p45[1], sp, qf[5]), 0.f), part);
    part = fmaf(a1.z, fmaxf(fmaf(p67[0], sp, qf[6]), 0.f), part);
    part = fmaf(a1.w, fmaxf(fmaf(p67[1], sp, qf[7]), 0.f), part);
    return part;
}

// PQ16 = 1: P' and Q are bf16 rows ([.., d] bf16, written by the projection GEMM's bf16 segments; BASELINE configs[4]); the lanes
// then span 8-channel pieces of them (one 16-byte load per row and lane at d <= 512) — h, X and the output stay fp32.
// PQ16 = 2: P' and Q are block-scaled OCP e4m3 rows (the GEMM's fp8 segments: one fp32 scale per 80-channel strip behind the
// row's d codes); a lane's piece is 8 codes (one 8-byte load) + its strip's scale; the score accumulates in fp32 as before.
template <int U, int PQ16, bool RADD, bool TRAIN = false>   // float4 pieces per lane: d <= 256 * U; RADD: K3 is added here (g.radd; 8 more
                                         // registers: 91 instead of 83 at U = 2, five waves per SIMD instead of six); TRAIN: see SparseArgs
__device__ __forceinline__ void xattn_sparse_centre(const SparseArgs& g, long rho, const int lane) {
    constexpr int V = (U + 1) / 2;         // 16-byte pieces of a bf16 row per lane
    constexpr int NBR = DIGAT_SPARSE_NBR;  // neighbour rows requested per step
    // wave-uniform values are made so explicitly (readfirstlane): row bases then live in SGPRs and every load is
    // "scalar base + lane offset" instead of 64-bit address arithmetic on the vector unit, which this kernel is bound by
    const int n = g.n, d4 = g.d4;
    if (rho >= (long)g.B * n) return;
    SP_T0();
    if (g.rowidx) {
        if (rho >= *g.nrows_dev) return;
        rho = __builtin_amdgcn_readfirstlane(g.rowidx[rho]);
    }
    SP_T(0);
    const long b = rho / n;
    const int i = (int)(rho - b * n);
    if (g.centre_limit > 0 && i >= g.centre_limit) return;
    // everything whose address is known now is requested in one go — live flag, group index, the two adjacency bytes of
    // this lane, a, X_i — with straight-line, clamped loads: a branch per load makes the compiler wait after each one, and
    // this kernel is a chain of global round trips per wave
    const float4* a4 = reinterpret_cast<const float4*>(g.a);
    const uint8_t* Ar = g.A + rho * n;
    const uint8_t lv = (g.live && !g.rowidx) ? g.live[rho] : (uint8_t)1;
    const int gi = g.group ? g.group[b] : 0;
    const uint8_t ab0 = Ar[min(lane, n - 1)], ab1 = Ar[min(lane + 64, n - 1)];
    float4 av[U], xin[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        const float4 aa = a4[c4];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();          // a = 0 on the padding channels: they add nothing
        if (!g.xgroup) xin[u] = reinterpret_cast<const float4*>(g.X)[rho * d4 + c4];
    }
    if (!__builtin_amdgcn_readfirstlane((int)lv)) return;
    const long gb = g.group ? (long)__builtin_amdgcn_readfirstlane(gi) : b;
    if (g.xgroup) {
#pragma unroll
        for (int u = 0; u < U; ++u) xin[u] = reinterpret_cast<const float4*>(g.X)[(gb * n + i) * d4 + min(lane + 64 * u, d4 - 1)];
    }
    unsigned c4l[U];                                       // this lane's float4 pieces (clamped: see above)
#pragma unroll
    for (int u = 0; u < U; ++u) c4l[u] = (unsigned)min(lane + 64 * u, d4 - 1);
    const float4* Pb = reinterpret_cast<const float4*>(g.P) + gb * n * d4;
    const float4* Hb = reinterpret_cast<const float4*>(g.h) + gb * n * d4;
    const float4* Qi = reinterpret_cast<const float4*>(g.Q) + (gb * n + i) * d4;
    // the adjacency row as two ballots (n <= 128)
    unsigned long long m[2];
    m[0] = __ballot(lane < n && ab0 != 0);
    m[1] = __ballot(lane + 64 < n && ab1 != 0);
    const int deg = __popcll(m[0]) + __popcll(m[1]);
    SP_T(1);
    float al[2] = {0.f, 0.f};          // lane l: alpha of neighbours l and 64 + l
    if (deg == 0) {                    // every score -1e9: uniform over all n nodes
        m[0] = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        m[1] = n > 64 ? (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull)) : 0ull;
        const float w = 1.f / (float)n;
        al[0] = lane < n ? w : 0.f;
        al[1] = lane + 64 < n ? w : 0.f;
    } else if (deg == 1) {             // a single neighbour (an isolated node's self loop): softmax of one value is 1
        al[0] = ((m[0] >> lane) & 1ull) ? 1.f : 0.f;
        al[1] = ((m[1] >> lane) & 1ull) ? 1.f : 0.f;
    } else {
        float4 q[U], r3[RADD ? U : 1];
        uint4 q16[PQ16 == 1 ? V : 1];
        float qf8[PQ16 == 2 ? V : 1][8];
        unsigned so8[PQ16 == 2 ? V : 1];     // byte offset of this lane's strip scale inside a row
        float4 a8[V][2];
        const int d8 = d4 >> 1;
        const uint4* Pb16 = reinterpret_cast<const uint4*>(g.P) + gb * n * d8;
        const unsigned char* Pb8 = reinterpret_cast<const unsigned char*>(g.P) + gb * n * g.ld8;
        if constexpr (PQ16 == 2) {
            const unsigned char* Qi8 = reinterpret_cast<const unsigned char*>(g.Q) + (gb * n + i) * g.ld8;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int c8 = min(lane + 64 * v, d8 - 1);
                so8[v] = (unsigned)(4 * d4 + 4 * (c8 / 10));
                const uint2 qc = *reinterpret_cast<const uint2*>(Qi8 + 8 * c8);
                const float sq = *reinterpret_cast<const float*>(Qi8 + so8[v]);
                const f2v q01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qc.x, false), q23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qc.x, true);
                const f2v q45 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qc.y, false), q67 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qc.y, true);
                qf8[v][0] = q01[0] * sq; qf8[v][1] = q01[1] * sq; qf8[v][2] = q23[0] * sq; qf8[v][3] = q23[1] * sq;
                qf8[v][4] = q45[0] * sq; qf8[v][5] = q45[1] * sq; qf8[v][6] = q67[0] * sq; qf8[v][7] = q67[1] * sq;
                const bool ok = lane + 64 * v < d8;
                a8[v][0] = ok ? a4[2 * c8] : f4_zero();          // a = 0 on the padding lanes: they add nothing
                a8[v][1] = ok ? a4[2 * c8 + 1] : f4_zero();
            }
        } else if constexpr (PQ16 == 1) {
            const uint4* Qi16 = reinterpret_cast<const uint4*>(g.Q) + (gb * n + i) * d8;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int c8 = min(lane + 64 * v, d8 - 1);
                q16[v] = Qi16[c8];
                const bool ok = lane + 64 * v < d8;
                a8[v][0] = ok ? a4[2 * c8] : f4_zero();          // a = 0 on the padding lanes: they add nothing
                a8[v][1] = ok ? a4[2 * c8 + 1] : f4_zero();
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c4 = min(lane + 64 * u, d4 - 1);
                q[u] = Qi[c4];
                if constexpr (RADD) r3[u] = (reinterpret_cast<const float4*>(g.radd) + b * d4)[c4];
            }
        }
        float sc[2] = {-INFINITY, -INFINITY};
        // the neighbours in ascending order, four per step, both ballots as one list (a history item's neighbours are its
        // category in the first ballot and often a single topic node in the second: a step per ballot would run half empty)
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 p[NBR][U];             // requests of empty slots repeat the first row (a cache hit); they are not computed
            uint4 p16[PQ16 == 1 ? NBR : 1][V];
            uint2 p8[PQ16 == 2 ? NBR : 1][V];
            float s8[PQ16 == 2 ? NBR : 1][V];
            if constexpr (PQ16 == 2) {
#pragma unroll
                for (int t = 0; t < NBR; ++t)
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const unsigned char* row = Pb8 + (long)j[t] * g.ld8;
                        p8[t][v] = *reinterpret_cast<const uint2*>(row + 8 * min(lane + 64 * v, d8 - 1));
                        s8[t][v] = *reinterpret_cast<const float*>(row + so8[v]);
                    }
            } else if constexpr (PQ16 == 1) {
#pragma unroll
                for (int t = 0; t < NBR; ++t)
#pragma unroll
                    for (int v = 0; v < V; ++v) p16[t][v] = (Pb16 + (long)j[t] * d8)[min(lane + 64 * v, d8 - 1)];
            } else {
#pragma unroll
                for (int t = 0; t < NBR; ++t)
#pragma unroll
                    for (int u = 0; u < U; ++u) p[t][u] = (Pb + (long)j[t] * d4)[c4l[u]];
            }
            SP_T(2);
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
                    float part = 0.f;
                    if constexpr (PQ16 == 2) {
#pragma unroll
                        for (int v = 0; v < V; ++v) part = score8_fp8(p8[t][v], s8[t][v], qf8[v], a8[v][0], a8[v][1], part);
                    } else if constexpr (PQ16 == 1) {
#pragma unroll
                        for (int v = 0; v < V; ++v) part = score8_bf16(p16[t][v], q16[v], a8[v][0], a8[v][1], part);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            float4 pk = p[t][u];
                            if constexpr (RADD) pk = f4_add(r3[u], pk);                           // K3 + K1, then + K2
                            part = fmaf(av[u].x, fmaxf(pk.x + q[u].x, 0.f), part);
                            part = fmaf(av[u].y, fmaxf(pk.y + q[u].y, 0.f), part);
                            part = fmaf(av[u].z, fmaxf(pk.z + q[u].z, 0.f), part);
                            part = fmaf(av[u].w, fmaxf(pk.w + q[u].w, 0.f), part);
                        }
                    }
                    const float e = wave_sum(part);
                    if constexpr (TRAIN) { if (lane == 0) g.t_spre[rho * n + j[t]] = e; }    // the score before leaky_relu (its derivative's sign)
                    const float lk = leaky02_uniform(e);                                       // leaky_relu(0.2)
                    if (lane == (j[t] & 63)) { if (j[t] < 64) sc[0] = lk; else sc[1] = lk; }
                }
            }
            SP_T(3);
        }
        const float mx = wave_max(fmaxf(sc[0], sc[1]));
        const float e0 = sc[0] > -INFINITY ? expf(sc[0] - mx) : 0.f;
        const float e1 = sc[1] > -INFINITY ? expf(sc[1] - mx) : 0.f;
        const float inv = wave_sum(e0 + e1);
        al[0] = e0 / inv;
        al[1] = e1 / inv;
        SP_T(4);
    }
    if constexpr (TRAIN) {
        // the whole alpha row (zero off the neighbours; uniform on an edgeless centre), then the attention dropout in place
        if (lane < n) g.t_alpha[rho * n + lane] = al[0];
        if (lane + 64 < n) g.t_alpha[rho * n + 64 + lane] = al[1];
        if (g.t_amask) {
            const unsigned thr = drop_threshold(g.t_p);
            const float scale = 1.f / (1.f - g.t_p);
            const bool k0 = lane < n && drop_keep(g.t_seed, rho * n + lane, thr);
            const bool k1 = lane + 64 < n && drop_keep(g.t_seed, rho * n + 64 + lane, thr);
            if (lane < n) g.t_amask[rho * n + lane] = k0;
            if (lane + 64 < n) g.t_amask[rho * n + 64 + lane] = k1;
            al[0] = k0 ? al[0] * scale : 0.f;
            al[1] = k1 ? al[1] * scale : 0.f;
        }
    }
    // aggregation over the same neighbours, ascending j: one fma chain per channel
    float4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f4_zero();
    {
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 hv[NBR][U];
#pragma unroll
            for (int t = 0; t < NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) hv[t][u] = (Hb + (long)j[t] * d4)[c4l[u]];
            SP_T(5);
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
                    const float w = j[t] < 64 ? lane_bcast(al[0], j[t]) : lane_bcast(al[1], j[t] - 64);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        acc[u].x = fmaf(w, hv[t][u].x, acc[u].x); acc[u].y = fmaf(w, hv[t][u].y, acc[u].y);
                        acc[u].z = fmaf(w, hv[t][u].z, acc[u].z); acc[u].w = fmaf(w, hv[t][u].w, acc[u].w);
                    }
                }
            }
            SP_T(6);
        }
    }
    if (g.fill_flags && !g.fill_flags[rho]) {
        float4* Fi = reinterpret_cast<float4*>(g.fill_out) + rho * d4;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (lane + 64 * u < d4) Fi[lane + 64 * u] = xin[u];
    }
    float4* Oi = reinterpret_cast<float4*>(g.out) + rho * d4;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = lane + 64 * u;
        if (c4 < d4) {
            const float4 x = xin[u];
            const float4 o = make_float4(fmaxf(acc[u].x, 0.f) + x.x, fmaxf(acc[u].y, 0.f) + x.y,
                                         fmaxf(acc[u].z, 0.f) + x.z, fmaxf(acc[u].w, 0.f) + x.w);
            Oi[c4] = o;
        }
    }
    SP_T(7);
#ifdef DIGAT_SPARSE_TIMERS
    if (sp_on && lane == 0) atomicAdd(g.timers + 8, 1ull);
#endif
}

// One wave per centre.  The grid covers every centre, or — guarded launches (run_if: the device decides between this kernel and
// the dense pair) — a fixed 2 048 workgroups that stride over the centres, so that the launch that is NOT wanted costs a
// couple of microseconds of empty workgroups instead of one per four centres.
// d <= 512 without K3 here: five waves per SIMD, 84 registers, no scratch.  (Round 2 forced six — 80 registers, two of them
// spilled — when that measured 5 % faster; with the kernels around it as they are now five is as fast or faster: 1.007-1.010
// against 1.02-1.03 ms per step, alternating runs.)
#ifndef DIGAT_SPARSE_WAVES
#define DIGAT_SPARSE_WAVES 5
#endif
template <int U, int PQ16, bool RADD, bool TRAIN = false>
__global__ void __launch_bounds__(256, (U <= 2 && !RADD) ? DIGAT_SPARSE_WAVES : 1) xattn_sparse_kernel(const SparseArgs g) {
    if (g.run_if && *g.run_if == 0) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // profiling: the live centres of the list; with a centre limit sparse_count_kernel adds the exact count instead (an atomic
    // per wave on one address costs ~15 ns each: 34 k of them more than doubled the launch)
    if (g.rowidx && g.exec_rows && g.exec_unit && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(g.exec_rows, (unsigned long long)*g.nrows_dev * g.exec_unit);
    const long total = (long)g.B * g.n;
    // The dispatcher deals workgroup ids round-robin to the 8 XCDs (id % 8), each with its own L2.  With xcd_group = G the ids
    // of a window of 8 G are permuted so that XCD x works on G CONSECUTIVE workgroups (4 G consecutive centres: the centres of
    // one graph, which share their neighbours' P' and h rows) while the windows keep the XCDs in step.
    unsigned blk = blockIdx.x;
    if (g.xcd_group > 0) {
        const unsigned G = (unsigned)g.xcd_group, w = blk / (8 * G), r = blk - w * 8 * G;
        blk = w * 8 * G + (r & 7) * G + (r >> 3);
    }
    for (long rho = (long)blk * 4 + wave; rho < total; rho += (long)gridDim.x * 4) xattn_sparse_centre<U, PQ16, RADD, TRAIN>(g, rho, lane);
}

// training: is this batch's adjacency sparse enough for the wave-per-centre kernel?  A sample of up to 16 graphs (a performance
// choice, never a correctness one): flag = 1 when they hold at most per_node entries per node on average.  One workgroup.
__global__ void __launch_bounds__(1024) train_sparse_decide_kernel(const uint8_t* A, int B, int n, int per_node, int* flag) {
    __shared__ int part[16];
    const int rows = min(B, 16), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long nn = (long)n * n;
    int s = 0;
    if (wave < rows) {                              // a wave per sampled graph: byte loads, sixteen in flight per lane
        const uint8_t* Ag = A + (((long)wave * B) / rows) * nn;
        for (long e0 = lane; e0 < nn; e0 += 64 * 16) {
            uint8_t v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = Ag[min(e0 + 64 * k, nn - 1)];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += (e0 + 64 * k < nn && v[k] != 0) ? 1 : 0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < 16; ++w) tot += part[w];
        *flag = tot <= per_node * rows * n ? 1 : 0;
    }
}
// ---- layer 0 of grouped rows: R rows of one impression per wave ------------------------------------------------------------------
// At layer 0 the rows of an impression share everything but K3: P, Q, h and the nodes X exist once per GROUP, the adjacency and
// the live centres are the group's.  The wave-per-centre kernel above still fetched the ~9 neighbour rows of P and of h once per
// (row, centre): 34 KB through the CU's L1 for every one of ~137 k centre-rows of a 4 096-row pass = 4.6 GB per launch against
// 64 B/clk/CU — the launch ran at half of what the L1 path can deliver (295 us) while moving a tenth of that from HBM.
// Here a wave owns centre i of up to R CONSECUTIVE rows of one group (a "chunk": lead[b] = rows led by row b, 0 = not a chunk's
// first row; sparse_l0_chunks_kernel): every P_j and h_j it fetches serves R rows (K3_b of the R rows sits in registers), so the
// L1 traffic per centre-row falls to about a third and the launch is bound by its arithmetic.  Per (row, centre) the operations
// and their order are those of xattn_sparse_centre<U, 0, true>: results are bit-identical.
struct SparseL0Args {
    SparseArgs g;
    const uint8_t* lead;     // [B]: rows led by row b (0: not a chunk's first row)
    const int* list;         // live centres b * n + i of the LEADING rows, ascending (live_list2_kernel's third list) ...
    const int* count;        // ... and how many
};

// one workgroup: gs[g] = first row of group g (groups must be runs of consecutive rows with consecutive ids: what the drivers
// build; anything else is detected and every row then leads a chunk of one, i.e. the per-row arithmetic without the sharing)
__global__ void __launch_bounds__(1024) sparse_l0_chunks_kernel(const int* row_group, int B, int G, int R, int* gs, uint8_t* lead) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 1024) {
        const int gb = row_group[b];
        if (gb < 0 || gb >= G) { bad = 1; continue; }
        if (b == 0) { if (gb != 0) bad = 1; gs[0] = 0; }
        else {
            const int gp = row_group[b - 1];
            if (gb == gp + 1) gs[gb] = b;
            else if (gb != gp) bad = 1;
        }
    }
    if (threadIdx.x == 0) gs[G] = B;
    __syncthreads();
    const bool contiguous = !bad && row_group[B - 1] == G - 1;
    for (int b = threadIdx.x; b < B; b += 1024) {
        int v = 1;
        if (contiguous) {
            const int gb = row_group[b];
            const int pos = b - gs[gb], left = gs[gb + 1] - b;
            v = (pos % R == 0) ? min(R, left) : 0;
        }
        lead[b] = (uint8_t)v;
    }
}

template <int U, int R>
__device__ __forceinline__ void xattn_sparse_l0_chunk(const SparseL0Args& a, const long k, const int lane);

template <int U, int R>
__global__ void __launch_bounds__(256, (U <= 2 && R <= 4) ? 4 : 1) xattn_sparse_l0_kernel(const SparseL0Args a) {      // four waves per SIMD: <= 128 registers
    const SparseArgs& g = a.g;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned blk = blockIdx.x;
    if (g.xcd_group > 0) {
        const unsigned Gx = (unsigned)g.xcd_group, w = blk / (8 * Gx), r = blk - w * 8 * Gx;
        blk = w * 8 * Gx + (r & 7) * Gx + (r >> 3);
    }
    // The grid is sized for the chunk count of contiguous groups (B / R + G chunks); when the row_group array is not such runs
    // (permuted or interleaved ids: sparse_l0_chunks_kernel then makes every row a chunk of one) the list is up to R times
    // longer than the grid: the waves stride over it.
    const long count = *a.count;
    for (long k = (long)blk * 4 + wave; k < count; k += (long)gridDim.x * 4) xattn_sparse_l0_chunk<U, R>(a, k, lane);
}

template <int U, int R>
__device__ __forceinline__ void xattn_sparse_l0_chunk(const SparseL0Args& a, const long k, const int lane) {
    constexpr int NBR = DIGAT_SPARSE_NBR;
    const SparseArgs& g = a.g;
    const long rho = __builtin_amdgcn_readfirstlane(a.list[k]);
    const int n = g.n, d4 = g.d4;
    const long b = rho / n;
    const int i = (int)(rho - b * n);
    const int nr = __builtin_amdgcn_readfirstlane((int)a.lead[b]);
    if (nr == 0) return;
    const long gb = (long)__builtin_amdgcn_readfirstlane(g.group[b]);
    const float4* a4 = reinterpret_cast<const float4*>(g.a);
    const uint8_t* Ar = g.A + rho * n;                       // the adjacency row of (b, i): the group's, whichever of its rows is asked
    const uint8_t ab0 = Ar[min(lane, n - 1)], ab1 = Ar[min(lane + 64, n - 1)];
    float4 av[U], xin[U], q[U], r3[R][U];
    unsigned c4l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        c4l[u] = (unsigned)c4;
        const float4 aa = a4[c4];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();
        q[u] = reinterpret_cast<const float4*>(g.Q)[(gb * n + i) * d4 + c4];
#pragma unroll
        for (int r = 0; r < R; ++r) r3[r][u] = reinterpret_cast<const float4*>(g.radd)[(b + min(r, nr - 1)) * d4 + c4];
    }
    const float4* Pb = reinterpret_cast<const float4*>(g.P) + gb * n * d4;
    const float4* Hb = reinterpret_cast<const float4*>(g.h) + gb * n * d4;
    unsigned long long m[2];
    m[0] = __ballot(lane < n && ab0 != 0);
    m[1] = __ballot(lane + 64 < n && ab1 != 0);
    const int deg = __popcll(m[0]) + __popcll(m[1]);
    float al[R][2];
    if (deg == 0) {                    // every score -1e9: uniform over all n nodes
        m[0] = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        m[1] = n > 64 ? (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull)) : 0ull;
        const float w = 1.f / (float)n;
#pragma unroll
        for (int r = 0; r < R; ++r) { al[r][0] = lane < n ? w : 0.f; al[r][1] = lane + 64 < n ? w : 0.f; }
    } else if (deg == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) { al[r][0] = ((m[0] >> lane) & 1ull) ? 1.f : 0.f; al[r][1] = ((m[1] >> lane) & 1ull) ? 1.f : 0.f; }
    } else {
        float sc[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r) { sc[r][0] = -INFINITY; sc[r][1] = -INFINITY; }
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 p[NBR][U];
#pragma unroll
            for (int t = 0; t < NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) p[t][u] = (Pb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (r < nr) {   // wave-uniform
                            float part = 0.f;
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const float4 pk = f4_add(r3[r][u], p[t][u]);                       // K3 + K1, then + K2
                                part = fmaf(av[u].x, fmaxf(pk.x + q[u].x, 0.f), part);
                                part = fmaf(av[u].y, fmaxf(pk.y + q[u].y, 0.f), part);
                                part = fmaf(av[u].z, fmaxf(pk.z + q[u].z, 0.f), part);
                                part = fmaf(av[u].w, fmaxf(pk.w + q[u].w, 0.f), part);
                            }
                            const float e = wave_sum(part);
                            const float lk = leaky02_uniform(e);                                   // leaky_relu(0.2)
                            if (lane == (j[t] & 63)) { if (j[t] < 64) sc[r][0] = lk; else sc[r][1] = lk; }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float mx = wave_max(fmaxf(sc[r][0], sc[r][1]));
            const float e0 = sc[r][0] > -INFINITY ? expf(sc[r][0] - mx) : 0.f;
            const float e1 = sc[r][1] > -INFINITY ? expf(sc[r][1] - mx) : 0.f;
            const float inv = wave_sum(e0 + e1);
            al[r][0] = e0 / inv;
            al[r][1] = e1 / inv;
        }
    }
    // the centre's own row X_i (the group's): requested here, behind the softmax, in registers the scoring phase has left — at the top
    // of the chunk it cost the kernel its fourth wave per SIMD once the reductions changed (129 registers); the offset passes
    // through an empty asm that reads an alpha so that the scheduler cannot hoist the request
    {
        unsigned xo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { xo[u] = c4l[u]; asm volatile("" : "+v"(xo[u]) : "v"(al[0][0])); }
#pragma unroll
        for (int u = 0; u < U; ++u) xin[u] = reinterpret_cast<const float4*>(g.X)[(gb * n + i) * d4 + xo[u]];
    }
    float4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = f4_zero();
    {
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 hv[NBR][U];
#pragma unroll
            for (int t = 0; t < NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) hv[t][u] = (Hb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (r < nr) {   // wave-uniform
                            const float w = j[t] < 64 ? lane_bcast(al[r][0], j[t]) : lane_bcast(al[r][1], j[t] - 64);
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                acc[r][u].x = fmaf(w, hv[t][u].x, acc[r][u].x); acc[r][u].y = fmaf(w, hv[t][u].y, acc[r][u].y);
                                acc[r][u].z = fmaf(w, hv[t][u].z, acc[r][u].z); acc[r][u].w = fmaf(w, hv[t][u].w, acc[r][u].w);
                            }
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < nr) {
            float4* Oi = reinterpret_cast<float4*>(g.out) + (rho + (long)r * n) * d4;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c4 = lane + 64 * u;
                if (c4 < d4) {
                    const float4 x = xin[u];
                    const float4 o = make_float4(fmaxf(acc[r][u].x, 0.f) + x.x, fmaxf(acc[r][u].y, 0.f) + x.y,
                                                 fmaxf(acc[r][u].z, 0.f) + x.z, fmaxf(acc[r][u].w, 0.f) + x.w);
                    Oi[c4] = o;
                }
            }
        }
    }
}

// ---- twins: up to TWIN_R centres of one graph with equal adjacency rows per wave -------------------------------------------------------
// Centres whose adjacency rows are equal have the same neighbours j (in a MIND user graph: the history items of one category), so
// the rows P'_j and h_j a wave fetches can serve all of them; only Q_i, X_i and the output row belong to the centre.  The
// wave-per-centre kernel fetched them once per centre (9 neighbours on average: 29 KB of a centre's 34 KB through the CU's L1).
// Per centre the operations and their order are those of xattn_sparse_centre<U, 0, false>: results are bit-identical.
// Round 5: the chunk's HEADER — its leading centre (twlist[k]), the twin word and the lane's two adjacency bytes: two dependent
// round trips before the first row request — arrives as arguments: the kernel's loop requests the header of a wave's NEXT chunk
// before it works on the current one (software pipeline, +5 registers).  The centres' own rows X_i are requested right after the
// softmax — their registers are the ones Q_i has just left — and arrive under the aggregation instead of costing a round trip of
// their own behind it.  Same operations in the same order per centre: bit-identical.
template <int U, int R>
__device__ __forceinline__ void xattn_sparse_twin_chunk(const SparseArgs& g, const long rho, const unsigned word, const uint8_t ab0, const uint8_t ab1,
                                                        const int lane) {
    constexpr int NBR = DIGAT_SPARSE_NBR;
    const int n = g.n, d4 = g.d4;
    const long b = rho / n;
    // the chunk's centres (ascending); with a centre limit the ones at or beyond it are not computed (nobody reads their rows)
    int mem[R], nr = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int mi = (int)((word >> (8 * r)) & 0xFFu);
        const bool ok = mi != 0xFF && (g.centre_limit <= 0 || mi < g.centre_limit);
        mem[r] = ok ? mi : mem[0];           // members are ascending: an invalid one is never followed by a valid one
        nr += ok ? 1 : 0;
        if (r == 0 && !ok) return;
    }
    const float4* a4 = reinterpret_cast<const float4*>(g.a);
    float4 av[U], q[R][U];
    unsigned c4l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c4 = min(lane + 64 * u, d4 - 1);
        c4l[u] = (unsigned)c4;
        const float4 aa = a4[c4];
        av[u] = lane + 64 * u < d4 ? aa : f4_zero();
#pragma unroll
        for (int r = 0; r < R; ++r) q[r][u] = reinterpret_cast<const float4*>(g.Q)[(b * n + mem[r]) * d4 + c4];
    }
    const float4* Pb = reinterpret_cast<const float4*>(g.P) + b * n * d4;
    const float4* Hb = reinterpret_cast<const float4*>(g.h) + b * n * d4;
    unsigned long long m[2];
    m[0] = __ballot(lane < n && ab0 != 0);
    m[1] = __ballot(lane + 64 < n && ab1 != 0);
    const int deg = __popcll(m[0]) + __popcll(m[1]);
    float al[R][2];
    if (deg == 0) {                    // every score -1e9: uniform over all n nodes
        m[0] = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        m[1] = n > 64 ? (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull)) : 0ull;
        const float w = 1.f / (float)n;
#pragma unroll
        for (int r = 0; r < R; ++r) { al[r][0] = lane < n ? w : 0.f; al[r][1] = lane + 64 < n ? w : 0.f; }
    } else if (deg == 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) { al[r][0] = ((m[0] >> lane) & 1ull) ? 1.f : 0.f; al[r][1] = ((m[1] >> lane) & 1ull) ? 1.f : 0.f; }
    } else {
        float sc[R][2];
#pragma unroll
        for (int r = 0; r < R; ++r) { sc[r][0] = -INFINITY; sc[r][1] = -INFINITY; }
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 p[NBR][U];
#pragma unroll
            for (int t = 0; t < NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) p[t][u] = (Pb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (r < nr) {   // wave-uniform
                            float part = 0.f;
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const float4 pk = p[t][u];
                                part = fmaf(av[u].x, fmaxf(pk.x + q[r][u].x, 0.f), part);
                                part = fmaf(av[u].y, fmaxf(pk.y + q[r][u].y, 0.f), part);
                                part = fmaf(av[u].z, fmaxf(pk.z + q[r][u].z, 0.f), part);
                                part = fmaf(av[u].w, fmaxf(pk.w + q[r][u].w, 0.f), part);
                            }
                            const float e = wave_sum(part);
                            const float lk = leaky02_uniform(e);                                   // leaky_relu(0.2)
                            if (lane == (j[t] & 63)) { if (j[t] < 64) sc[r][0] = lk; else sc[r][1] = lk; }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float mx = wave_max(fmaxf(sc[r][0], sc[r][1]));
            const float e0 = sc[r][0] > -INFINITY ? expf(sc[r][0] - mx) : 0.f;
            const float e1 = sc[r][1] > -INFINITY ? expf(sc[r][1] - mx) : 0.f;
            const float inv = wave_sum(e0 + e1);
            al[r][0] = e0 / inv;
            al[r][1] = e1 / inv;
        }
    }
    // The centres' own rows X_i.  All R of them in front of the aggregation would arrive under it, but their 32 registers do not
    // fit beside acc + h rows at four waves per SIMD (round 4: 134 registers; round 5 with the pipelined header: 8 spilled).  The
    // LEADING centre's row does (8 registers), and most chunks have no other member (1.7 centres per chunk on MIND-shaped users):
    // it is requested here, behind the softmax — the offset passes through an empty asm that reads an alpha, so that the scheduler
    // cannot hoist the request into the scoring phase — and the followers' rows keep their round trip behind the aggregation,
    // which a chunk of one no longer pays.
    float4 xin[R][U];
    {
        unsigned xo[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { xo[u] = c4l[u]; asm volatile("" : "+v"(xo[u]) : "v"(al[0][0])); }
#pragma unroll
        for (int u = 0; u < U; ++u) xin[0][u] = reinterpret_cast<const float4*>(g.X)[(b * n + mem[0]) * d4 + xo[u]];
    }
    float4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = f4_zero();
    {
        unsigned long long m0 = m[0], m1 = m[1];
        while (m0 | m1) {
            int j[NBR], cnt = 0;
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (m0) { j[t] = __builtin_ctzll(m0); m0 &= m0 - 1ull; ++cnt; }
                else if (m1) { j[t] = 64 + __builtin_ctzll(m1); m1 &= m1 - 1ull; ++cnt; }
                else j[t] = j[0];
            }
            float4 hv[NBR][U];
#pragma unroll
            for (int t = 0; t < NBR; ++t)
#pragma unroll
                for (int u = 0; u < U; ++u) hv[t][u] = (Hb + (long)j[t] * d4)[c4l[u]];
#pragma unroll
            for (int t = 0; t < NBR; ++t) {
                if (t < cnt) {          // wave-uniform
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (r < nr) {   // wave-uniform
                            const float w = j[t] < 64 ? lane_bcast(al[r][0], j[t]) : lane_bcast(al[r][1], j[t] - 64);
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                acc[r][u].x = fmaf(w, hv[t][u].x, acc[r][u].x); acc[r][u].y = fmaf(w, hv[t][u].y, acc[r][u].y);
                                acc[r][u].z = fmaf(w, hv[t][u].z, acc[r][u].z); acc[r][u].w = fmaf(w, hv[t][u].w, acc[r][u].w);
                            }
                        }
                    }
                }
            }
        }
    }
    if (nr > 1) {      // wave-uniform: one branch around all the followers' requests
#pragma unroll
        for (int r = 1; r < R; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) xin[r][u] = reinterpret_cast<const float4*>(g.X)[(b * n + mem[r]) * d4 + c4l[u]];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < nr) {
            float4* Oi = reinterpret_cast<float4*>(g.out) + (b * n + mem[r]) * d4;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c4 = lane + 64 * u;
                if (c4 < d4) {
                    const float4 x = xin[r][u];
                    const float4 o = make_float4(fmaxf(acc[r][u].x, 0.f) + x.x, fmaxf(acc[r][u].y, 0.f) + x.y,
                                                 fmaxf(acc[r][u].z, 0.f) + x.z, fmaxf(acc[r][u].w, 0.f) + x.w);
                    Oi[c4] = o;
                }
            }
        }
    }
}

// the grid is capped (the number of leading centres is known on the device only): a wave strides over the list
#ifndef DIGAT_TWIN_WAVES
#define DIGAT_TWIN_WAVES (DIGAT_TWIN_R <= 2 ? 5 : 4)   // TWIN_R = 2: 94 registers, five waves per SIMD; 4: 114 registers, four (five would spill 10)
#endif
// DIGAT_TWIN_WPG (waves per workgroup): digat_xattn_plan.h, with the grid
template <int U, int R>
__global__ void __launch_bounds__(64 * DIGAT_TWIN_WPG, U <= 2 ? DIGAT_TWIN_WAVES : 1) xattn_sparse_twin_kernel(const SparseArgs g) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (g.exec_rows && g.exec_unit && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(g.exec_rows, (unsigned long long)*g.nrows_dev * g.exec_unit);
    unsigned blk = blockIdx.x;
    if (g.xcd_group > 0) {
        const unsigned Gx = (unsigned)g.xcd_group, w = blk / (8 * Gx), r = blk - w * 8 * Gx;
        blk = w * 8 * Gx + (r & 7) * Gx + (r >> 3);
    }
    const long count = *g.twcount;
    const long stride = (long)gridDim.x * DIGAT_TWIN_WPG;
    long k = (long)blk * DIGAT_TWIN_WPG + wave;
    if (k >= count) return;
    const int n = g.n;
    // software pipeline over the wave's chunks: header of chunk k in hand, leading centre of chunk k + stride in flight
    long rho = __builtin_amdgcn_readfirstlane(g.twlist[k]);
    unsigned word_v = g.twin[rho];
    uint8_t ab0 = g.A[rho * n + min(lane, n - 1)], ab1 = g.A[rho * n + min(lane + 64, n - 1)];
    int rho_next_v = g.twlist[min(k + stride, count - 1)];
    for (;;) {
        const long kn = k + stride;
        const bool more = kn < count;
        // the next chunk's word and adjacency bytes (its leading centre was requested one chunk ago) and the leading centre of the one after
        const long rho_n = more ? (long)__builtin_amdgcn_readfirstlane(rho_next_v) : rho;
        const unsigned word_n = g.twin[rho_n];
        const uint8_t ab0_n = g.A[rho_n * n + min(lane, n - 1)], ab1_n = g.A[rho_n * n + min(lane + 64, n - 1)];
        rho_next_v = g.twlist[min(kn + stride, count - 1)];
        xattn_sparse_twin_chunk<U, R>(g, rho, (unsigned)__builtin_amdgcn_readfirstlane((int)word_v), ab0, ab1, lane);
        if (!more) break;
        k = kn; rho = rho_n; word_v = word_n; ab0 = ab0_n; ab1 = ab1_n;
    }
}

// profiling only: the algorithmic bytes of a row-list launch with a centre limit — the centres below the limit are
// computed (`unit` bytes each: P'_j, h_j as some centre's neighbour, Q_i, X_i, the output row, the adjacency row), the live nodes
// at or beyond it only serve as neighbours (`unit_nbr`: their P' and h rows)
__global__ void __launch_bounds__(1024) sparse_count_kernel(const int* rowidx, const int* nrows_dev, int n, int limit, unsigned unit, unsigned unit_nbr,
                                                            unsigned long long* out) {
    __shared__ int part[16], part2[16];
    const int total = *nrows_dev;
    int lo = 0, hi = 0;           // centres below the limit / list entries this workgroup looked at (64 workgroups: the one-workgroup form
                                  // took 38 us and sat in front of the launch it prices)
    for (int k = blockIdx.x * 1024 + threadIdx.x; k < total; k += gridDim.x * 1024) { lo += (rowidx[k] % n) < limit; ++hi; }
    for (int o = 32; o > 0; o >>= 1) { lo += __shfl_xor(lo, o, 64); hi += __shfl_xor(hi, o, 64); }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = lo; part2[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long t = 0, m = 0;
        for (int w = 0; w < 16; ++w) { t += part[w]; m += part2[w]; }
        if (m) atomicAdd(out, (unsigned long long)t * unit + (unsigned long long)(m - t) * unit_nbr);
    }
}

// profiling only: the algorithmic bytes of layer 0 of GROUPED rows on the live lists.  P, Q, h and X exist once per
// group — 4 rows + the adjacency row per live node of a group — and every live (row, centre) writes one output row.  Groups are
// runs of equal ids (anything else: every change of id counts as a new group, an upper bound).
__global__ void __launch_bounds__(1024) sparse_l0_bytes_kernel(const uint8_t* live, const int* row_group, int B, int n, unsigned row_bytes,
                                                               unsigned long long* out) {
    __shared__ unsigned long long part[16];
    unsigned long long c = 0;
    for (int b = blockIdx.x * 1024 + threadIdx.x; b < B; b += gridDim.x * 1024) {
        int lv = 0;
        for (int i = 0; i < n; ++i) lv += live[(long)b * n + i] != 0;
        const bool first = b == 0 || row_group[b] != row_group[b - 1];
        c += (unsigned long long)lv * row_bytes + (first ? (unsigned long long)lv * (4ull * row_bytes + n) : 0ull);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < 16; ++w) t += part[w];
        atomicAdd(out, t);
    }
}

// Algorithmic bytes of one sparse Eq. 8 launch = what has to cross HBM once (DESIGN.md section 5):
//  * plain: SURVEY 8d's bytes_B = B (5 n d 4 + n^2) + 4 d — P', Q, h, X in, the nodes out, the adjacency (+ B d 4 when K3 joins here);
//  * layer 0 of grouped rows: P, Q, h (and X with xgroup) exist once per GROUP, so only G n d 4 bytes each are distinct;
//  * with a live-row list only the live centres are read or written — and every neighbour of a live centre is a live node.
//    Layers >= 1 (rows of their own): (5 d 4 + n) bytes per live centre.  Layer 0 of grouped rows: 4 rows + the adjacency row per
//    live node of a GROUP, one output row per live (row, centre), K3 per row (sparse_l0_bytes_kernel).  The counts are known on the
//    device only: the launch (or a one-workgroup counting kernel in front of it) adds the BYTES to a device counter of its part and
//    digat_profile_stop reads it; the launch itself is recorded with what the host knows (the 4 d of `a`, K3).
static double sparse_bytes(const SparseArgs& g) {
    const double row = (double)g.d4 * 16;
    if (g.rowidx) return row + (g.radd ? (double)g.B * row : 0.0);
    double bytes = (double)g.B * g.n * g.n + row + (g.radd ? (double)g.B * row : 0.0);
    const double rows_b = (double)g.B * g.n, rows_g = (double)(g.group && g.G > 0 ? g.G : g.B) * g.n;
    bytes += 3.0 * rows_g * row;                                  // P, Q, h
    bytes += (g.group && g.xgroup ? rows_g : rows_b) * row;       // X
    bytes += rows_b * row;                                        // out
    return bytes;
}
// which Eq. 8 kernel a sparse launch is, for the per-part profile (XPART_*)
static int sparse_part(const SparseArgs& g) { return g.prof_part ? g.prof_part - 1 : (g.rowidx ? (g.group ? XPART_L0 : XPART_TWIN) : XPART_OTHER); }
// the device-side byte count of a row-list launch (profiling only): in the kernel (count x unit) or by a counting kernel in front
static int sparse_prof_bytes(SparseArgs& g, hipStream_t st) {
    g.exec_rows = nullptr; g.exec_unit = 0;
    if (!g.rowidx || !g_prof.enabled || !((g_prof.kind_mask >> DIGAT_KERNEL_XATTN) & 1u)) return DIGAT_OK;
    const unsigned row = (unsigned)g.d4 * 16;
    g.exec_rows = g_prof.rows_dev + 8 + sparse_part(g);
    // bf16 P', Q: half a row each; e4m3: a quarter + the strip scales
    const unsigned unit = g.pq16 == 2 ? (unsigned)(3.5 * row + 2.0 * 4 * (g.d4 / 20) + g.n) : (g.pq16 ? 4u : 5u) * row + (unsigned)g.n;
    if (g.group && g.live && !g.prof_part) {
        hipLaunchKernelGGL(sparse_l0_bytes_kernel, dim3((g.B + 1023) / 1024), dim3(1024), 0, st, g.live, g.group, g.B, g.n, row, g.exec_rows);
        DIGAT_CHECK_LAUNCH();
    } else if (g.centre_limit > 0) {
        hipLaunchKernelGGL(sparse_count_kernel, dim3(64), dim3(1024), 0, st, g.rowidx, g.nrows_dev, g.n, g.centre_limit, unit,
                           g.pq16 ? row + row / (g.pq16 == 2 ? 4 : 2) : 2 * row, g.exec_rows);
        DIGAT_CHECK_LAUNCH();
    } else {
        g.exec_unit = unit;
    }
    return DIGAT_OK;
}

#ifdef DIGAT_SPARSE_TIMERS
static unsigned long long* g_sparse_timers = nullptr;
extern "C" int digat_debug_sparse_timers(double* out9) {
    if (!g_sparse_timers || !out9) return DIGAT_ERR_ARG;
    unsigned long long h[9];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, g_sparse_timers, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return DIGAT_ERR_LAUNCH;
    for (int k = 0; k < 9; ++k) out9[k] = (double)h[k];
    (void)hipMemset(g_sparse_timers, 0, 16 * 8);
    return DIGAT_OK;
}
#endif
// SparseArgs with its mandatory fields; everything optional is off until the caller sets it by name
static SparseArgs sparse_args(const float* P, const float* Q, const float* h, const float* X, const float* a, const uint8_t* A, float* out,
                              int B, int n, int d4) {
    SparseArgs g = {};
    g.P = P; g.Q = Q; g.h = h; g.X = X; g.a = a; g.A = A; g.out = out; g.B = B; g.n = n; g.d4 = d4;
    return g;
}
// what the routes of digat_xattn_plan.h ask about a launch: its sizes, and which optional fields were passed
static Eq8SparseIn sparse_in(const SparseArgs& g) {
    Eq8SparseIn in = {};
    in.B = g.B; in.n = g.n; in.d4 = g.d4;
    in.radd = g.radd != nullptr; in.group = g.group != nullptr; in.xgroup = g.xgroup != 0; in.live = g.live != nullptr;
    in.run_if = g.run_if != nullptr; in.fill_flags = g.fill_flags != nullptr; in.rowidx = g.rowidx != nullptr; in.nrows_dev = g.nrows_dev != nullptr;
    in.twin = g.twin && g.twlist && g.twcount;
    in.pq16 = g.pq16; in.centre_limit = g.centre_limit; in.ld8 = g.ld8;
    return in;
}
// every launch of xattn_sparse_kernel: the route's instantiation on the route's grid
static void launch_sparse_kernel(const Eq8Launch& l, const SparseArgs& g, hipStream_t st) {
    eq8_by_width<4>(l.U, [&](auto u) {
        constexpr int U = decltype(u)::value;
        const dim3 grid(l.grid), block(l.block);
        if (l.train) hipLaunchKernelGGL((xattn_sparse_kernel<U, 0, false, true>), grid, block, 0, st, g);
        else if (l.pq16 == 2) hipLaunchKernelGGL((xattn_sparse_kernel<U, 2, false>), grid, block, 0, st, g);
        else if (l.pq16 == 1) hipLaunchKernelGGL((xattn_sparse_kernel<U, 1, false>), grid, block, 0, st, g);
        else if (l.radd) hipLaunchKernelGGL((xattn_sparse_kernel<U, 0, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((xattn_sparse_kernel<U, 0, false>), grid, block, 0, st, g);
    });
}
// the sparse arm of an inference layer: the twin kernel or the wave-per-centre kernel (eq8_sparse_route)
static int launch_sparse(const SparseArgs& g_in, hipStream_t st) {
    const Eq8SparseRoute r = eq8_sparse_route(sparse_in(g_in));
    if (r.status) return r.status;
    const Eq8Launch& l = r.launch;
    SparseArgs g = g_in;
    { const int rcp = sparse_prof_bytes(g, st); if (rcp) return rcp; }
    ProfScope prof(DIGAT_KERNEL_XATTN, sparse_bytes(g), st, 0.0, sparse_part(g));
    g.xcd_group = l.xcd_group;
#ifdef DIGAT_SPARSE_TIMERS
    if (!g_sparse_timers && hipMalloc((void**)&g_sparse_timers, 16 * 8) == hipSuccess) (void)hipMemset(g_sparse_timers, 0, 16 * 8);
    g.timers = g.rowidx ? g_sparse_timers : nullptr;          // the user graph's row-list launches
#endif
    if (l.kernel == EQ8_TWIN)
        eq8_by_width<2>(l.U, [&](auto u) {
            hipLaunchKernelGGL((xattn_sparse_twin_kernel<decltype(u)::value, TWIN_R>), dim3(l.grid), dim3(l.block), 0, st, g);
        });
    else launch_sparse_kernel(l, g, st);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// layer 0 of grouped rows on the chunk kernel (see xattn_sparse_l0_kernel; `l` from eq8_l0_route, where the launch is eligible);
// `lead` from sparse_l0_chunks_kernel
constexpr int SPARSE_L0_ROWS = DIGAT_L0_ROWS;
static int launch_sparse_l0(const SparseArgs& g_in, const Eq8Launch& l, const uint8_t* lead, const int* list, const int* count, hipStream_t st) {
    SparseL0Args a{g_in, lead, list, count};
    SparseArgs& g = a.g;
    { const int rcp = sparse_prof_bytes(g, st); if (rcp) return rcp; }
    ProfScope prof(DIGAT_KERNEL_XATTN, sparse_bytes(g), st, 0.0, XPART_L0);
    g.xcd_group = l.xcd_group;
    eq8_by_width<2>(l.U, [&](auto u) {
        hipLaunchKernelGGL((xattn_sparse_l0_kernel<decltype(u)::value, SPARSE_L0_ROWS>), dim3(l.grid), dim3(l.block), 0, st, a);
    });
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// Aggregation kernel: out[b] = relu(alpha[b] @ h[b]) + X[b] on the fp32 matrix cores
// (v_mfma_f32_16x16x4_f32 is an exact k-ordered fma chain, so this equals a sequential sum over the
// neighbours j).  One workgroup owns one row b: alpha[b] (n*n floats) is staged in LDS once, each wave
// owns 64 channels: MFMA column l&15 of channel tile s stands for channel c0 + 4*(l&15) + s, so a lane
// loads h as one float4 and stores its 4 results as one float4.  h rows are requested AG_PF neighbour
// steps ahead; alpha blocks (16 centres x 4 neighbours) that are entirely zero — masked pairs — skip
// their MFMAs.
struct AggArgs {
    const float* alpha; const float* Hh; const float* X; float* out; int B, n, d, groups, sa;
    const uint8_t* live;     // optional [B,n]: rows of dead nodes (see user_live_flags_kernel) are neither read nor written
    const int* hgroup;       // optional [B]: row b's h lives at Hh[hgroup[b]]
    const int* skip_if;      // optional device int: the launch returns at once when *skip_if != 0
};
constexpr int AG_IT = 5;     // 16-row centre tiles per pass (80 centres)
constexpr int AG_PF = 3;     // neighbour steps of h in flight

template <int MAXT>      // the largest workgroup of the instantiation (64 x ceil(d / 64) threads): see topic_pool_resident_kernel
__global__ void __launch_bounds__(MAXT) xattn_agg_kernel(const AggArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (g.skip_if && *g.skip_if != 0) return;
    float* As = reinterpret_cast<float*>(smem);            // [n][sa], sa odd: conflict-free column reads
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int n = g.n, d = g.d, sa = g.sa;
    unsigned char* lv = smem + (size_t)n * sa * 4;         // [n] live flags of this row's nodes (all 1 without a list)
    for (int i = tid; i < n; i += blockDim.x) lv[i] = g.live ? g.live[(long)b * n + i] : 1;
    __syncthreads();
    {
        // a dead node's alpha row is never used (its output is not written) and its column is zero for every live
        // centre (it has no edge to them): zero rows in the image let whole MFMA blocks drop out
        const float* Ab = g.alpha + (long)b * n * n;
        for (int e = tid; e < n * n; e += blockDim.x) {
            const int i = e / n, j = e - i * n;
            As[i * sa + j] = lv[i] ? Ab[e] : 0.f;
        }
    }
    __syncthreads();
    const int lr = lane & 15, lq = lane >> 4;
    // a wave per 64 channels; beyond 1024 channels (more groups than the 16 waves of the largest workgroup) a wave takes several in turn
    for (int cg = wave; cg < g.groups; cg += (int)(blockDim.x >> 6)) {
        const int ch = cg * 64 + 4 * lr;
        const bool ch_ok = ch < d;
        const float* Hb = g.Hh + (long)(g.hgroup ? g.hgroup[b] : b) * n * d;
        const float* Xb = g.X + (long)b * n * d;
        float* Ob = g.out + (long)b * n * d;
        const int nit = (n + 15) >> 4;
        const int nsteps = (n + 3) >> 2;

        auto load_h = [&](int step) -> float4 {
            const int j = step * 4 + lq;
            return (j < n && ch_ok && lv[j]) ? *reinterpret_cast<const float4*>(Hb + (long)j * d + ch) : f4_zero();
        };

        for (int it0 = 0; it0 < nit; it0 += AG_IT) {
            v4f acc[AG_IT][4];
    #pragma unroll
            for (int it = 0; it < AG_IT; ++it)
    #pragma unroll
                for (int s = 0; s < 4; ++s) acc[it][s] = (v4f){0.f, 0.f, 0.f, 0.f};

            float4 hq[AG_PF];
    #pragma unroll
            for (int u = 0; u < AG_PF; ++u) hq[u] = load_h(u);
            for (int step = 0; step < nsteps; step += AG_PF) {
    #pragma unroll
                for (int u = 0; u < AG_PF; ++u) {
                    const int st = step + u;
                    if (st < nsteps) {
                        const float4 hc = hq[u];
                        hq[u] = load_h(st + AG_PF);
                        const int j = st * 4 + lq;
    #pragma unroll
                        for (int it = 0; it < AG_IT; ++it) {
                            const int i = (it0 + it) * 16 + lr;
                            const float av = (i < n && j < n) ? As[i * sa + j] : 0.f;
                            if (it0 + it < nit && __any(av != 0.f)) {
                                acc[it][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hc.x, acc[it][0], 0, 0, 0);
                                acc[it][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hc.y, acc[it][1], 0, 0, 0);
                                acc[it][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hc.z, acc[it][2], 0, 0, 0);
                                acc[it][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, hc.w, acc[it][3], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            if (ch_ok) {
    #pragma unroll
                for (int it = 0; it < AG_IT; ++it) {
    #pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = (it0 + it) * 16 + 4 * lq + r;
                        if (i < n && lv[i]) {
                            const float4 x = *reinterpret_cast<const float4*>(Xb + (long)i * d + ch);
                            *reinterpret_cast<float4*>(Ob + (long)i * d + ch) =
                                make_float4(fmaxf(acc[it][0][r], 0.f) + x.x, fmaxf(acc[it][1][r], 0.f) + x.y,
                                            fmaxf(acc[it][2][r], 0.f) + x.z, fmaxf(acc[it][3][r], 0.f) + x.w);
                        }
                    }
                }
            }
        }
    }
}
// AggArgs with its mandatory fields (groups and sa come from the route: launch_agg)
static AggArgs agg_args(const float* alpha, const float* h, const float* X, float* out, int B, int n, int d) {
    AggArgs ag = {};
    ag.alpha = alpha; ag.Hh = h; ag.X = X; ag.out = out; ag.B = B; ag.n = n; ag.d = d;
    return ag;
}
// every launch of it (eq8_agg_route)
static int launch_agg(AggArgs ag, const Eq8AggRoute& r, hipStream_t st) {
    if (r.status) return r.status;
    const Eq8Launch& l = r.launch;
    ag.groups = r.groups; ag.sa = r.sa;
    if (l.maxt == 512) hipLaunchKernelGGL(xattn_agg_kernel<512>, dim3(l.grid), dim3(l.block), l.lds, st, ag);
    else hipLaunchKernelGGL(xattn_agg_kernel<1024>, dim3(l.grid), dim3(l.block), l.lds, st, ag);
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// the score launch of a route (eq8_score_launch): a small-graph kernel, or the tile kernel on the plan `g` was made from
static int launch_score(const Eq8Launch& l, const ScoreArgs& g, hipStream_t st) {
    const dim3 grid(l.grid), block(l.block);
    if (l.kernel == EQ8_SMALL_LDS)
        eq8_by_width<4>(l.U, [&](auto u) { hipLaunchKernelGGL(xattn_small_lds_kernel<decltype(u)::value>, grid, block, l.lds, st, g); });
    else if (l.kernel == EQ8_SMALL)
        eq8_by_width<4>(l.U, [&](auto u) { hipLaunchKernelGGL(xattn_score_small_kernel<decltype(u)::value>, grid, block, 0, st, g); });
    else {
        if (l.raise_lds) {
            static int raised = 0;     // benign race: the attribute is idempotent
            if (!raised) {
                if (hipFuncSetAttribute((const void*)xattn_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        160 * 1024) != hipSuccess) return DIGAT_ERR_LAUNCH;
                raised = 1;
            }
        }
        hipLaunchKernelGGL(xattn_score_kernel, grid, block, l.lds, st, g);
    }
    DIGAT_CHECK_LAUNCH();
    return DIGAT_OK;
}

// launch_xattn_pairwise's optional inputs; what a caller does not set stays off
struct PairOpts {
    const uint8_t* live = nullptr;         // [B,n]: dead nodes are neither scored nor aggregated
    const int* group = nullptr;            // [B]: Q and h of row b live at row group[b]
    const float* radd = nullptr;           // [B,d] (small graphs): Pr holds K1 alone, K3 is added in the kernel
    bool alpha_wanted = true;              // false: small graphs are scored and aggregated in one launch, alpha is not written
    const int* skip_if = nullptr;          // device int: both launches return at once when it is != 0 (the sparse kernel does this batch)
    const int64_t* bindex = nullptr;       // [B] (fused small-graph form): Pr, Q, h, X are tables, row b's graph is their row bindex[b]
};
// Pr = K3 + K1 (r already added to the neighbour-side projection), see xattn_core
static int launch_xattn_pairwise(const float* Pr, const float* Q, const float* h, const float* X,
                                 const float* a, const uint8_t* A, float* out, float* alpha,
                                 int B, int n, int d, hipStream_t st, const PairOpts& o = PairOpts()) {
    Eq8PairIn in = {};
    in.B = B; in.n = n; in.d = d; in.alpha_wanted = o.alpha_wanted; in.live = o.live != nullptr; in.group = o.group != nullptr;
    in.radd = o.radd != nullptr; in.bindex = o.bindex != nullptr; in.guarded = o.skip_if != nullptr;
    const Eq8PairRoute r = eq8_pair_route(in);
    if (r.status || r.score.kernel == EQ8_NONE) return r.status;
    ScoreArgs g = score_args(r.tile);
    g.P = Pr; g.Q = Q; g.a = a; g.A = A; g.alpha = alpha; g.live = o.live; g.qgroup = o.group; g.radd = o.radd; g.bindex = o.bindex;
    g.skip_if = o.skip_if;            // guarded launches (the device decides between them and the sparse kernel) carry no nominal work
    if (r.fused) { g.agg_h = h; g.agg_x = X; g.agg_out = out; }
    {
        // algorithmic bytes of the score launch: P', Q in (2 n d floats), adjacency, alpha out, a (SURVEY 8d bytes_A);
        // the fused small-graph launch also aggregates: P', Q, h, X in, the nodes out, K3, adjacency (bytes_B)
        const double bytes = r.fused ? (double)B * (5.0 * n * d * 4 + (o.radd ? 4.0 * d : 0.0) + (double)n * n) + 4.0 * d
                                     : (double)B * (2.0 * n * d * 4 + (double)n * n * 5.0) + 4.0 * d;
        ProfScope prof(DIGAT_KERNEL_XATTN, o.skip_if ? 0.0 : bytes, st, 0.0, r.fused ? XPART_NEWS : XPART_OTHER);
        const int rc2 = launch_score(r.score, g, st);
        if (rc2) return rc2;
    }
    if (!r.fused) {
        AggArgs ag = agg_args(alpha, h, X, out, B, n, d);
        ag.live = o.live; ag.hgroup = o.group; ag.skip_if = o.skip_if;
        // algorithmic bytes of the aggregation launch: h, X in + out (3 n d floats), alpha in;
        // flops 2 n^2 d per row run on the MFMA pipe
        ProfScope prof(DIGAT_KERNEL_AGG, o.skip_if ? 0.0 : (double)B * (3.0 * n * d * 4 + (double)n * n * 4.0), st);
        return launch_agg(ag, r.agg, st);
    }
    return DIGAT_OK;
}
