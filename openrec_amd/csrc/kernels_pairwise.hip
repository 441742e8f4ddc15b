// Fused pairwise (BPR / UCML) train-step kernels for gfx950 (MI355X, CDNA4).
//
// Replaces, for one batch of B (user, pos item, neg item) triplets, the TF op
// sequence that the reference makes TensorFlow run (paths relative to
// /root/reference):
//   5 Embedding gathers                      recommenders/bpr.py:23-27, ucml.py:23-27
//   dot / L2-distance score, bias add        modules/pairwise_log_loss.py:19-30, ucml.py:29-37
//   clamp, log-sigmoid mean | hinge sum      pairwise_log_loss.py:32 | ucml.py:39
//   l2_loss                                  bpr.py:35, ucml.py:40
//   GradientTape over (loss, l2_loss)        tf2_examples/bpr_citeulike.py:35-37
//   Keras optimizer sparse apply             tf2_examples/bpr_citeulike.py:38
//
// Design (DESIGN.md has the measurements behind each choice):
//   * The step is bound by the number of random memory transactions, not by
//     flops: 3 row reads + 3 row writes per triplet with no reuse.  A row of D
//     fp32 is owned by LPR = D/4 adjacent lanes (one float4 each): a D=64 row is
//     one coalesced 256-B segment, a wavefront carries 64/LPR triplets, and the
//     dot products reduce inside the lane group with DPP (quad_perm,
//     row_half_mirror, row_mirror) -- no LDS, no barriers in the hot kernel.
//   * TF takes every gradient of a step on the PRE-step tables.  A one-pass
//     in-place kernel breaks that only for rows referenced more than once in the
//     batch.  Per-row metadata in HBM would cost one extra random transaction
//     per reference (measured: about as expensive as a row access), so duplicates
//     are found WITHOUT touching HBM tables:
//       dedup_kernel    : row-range buckets of 425984 rows; each workgroup keeps
//                         three LDS bitmaps ("seen", "seen twice", "seen three
//                         times", 156 KiB) for its range while streaming the
//                         L2-resident id arrays: exact, no hashing, no overflow.
//                         It runs once for ALL K steps of a call, before the
//                         first step.  Output per step: the ids rewritten with
//                         the duplicate flag in bit 31 and the reference's role
//                         (first / second / any of >= 3) in bits 30:29, and the
//                         list of duplicated rows.
//       fused_kernel    : unique rows are read, scored and updated in place
//                         (exact: nobody else reads or writes them).  A
//                         duplicated row is left untouched; a reference to it
//                         deposits its gradient in scratch: rows referenced
//                         exactly twice (the vast majority) get ONE PLAIN STORE
//                         per reference into scratch row 1 / scratch row 2 (no
//                         atomics, bitwise reproducible), rows referenced >= 3
//                         times use fire-and-forget fp32 atomics into scratch row 1.
//       dup_apply_kernel: for every duplicated row of the step, apply the
//                         optimizer rule once with the summed gradient (TF's
//                         dedup-sum semantics for Adagrad; identical for SGD)
//                         and re-zero the scratch rows.
//     The scratch tables are all-zero between steps.
#include "orx_internal.h"

#include "orx_device.h"

// ------------------------------------------------------------ dedup kernel ---
// One workgroup per (step, table, 425984-row range).  Exact duplicate detection
// on the id arrays alone: three LDS bitmaps over the rows of the range; the ids of
// the step are streamed twice from L2 (mark, then emit).  No HBM table is touched.
constexpr int DD_WORDS = 13312;                 // 32-bit words per bitmap
constexpr int DD_ROWS = DD_WORDS * 32;          // rows covered by one workgroup (425984)
constexpr int DD_THREADS = 1024;
constexpr int DD_LDS_BYTES = 3 * DD_WORDS * 4;  // three bitmaps: seen / seen twice / seen three times (156 KiB of the 160 KiB LDS)

// visit every reference j in [0, n) of a table's id stream (segment A of length nA, then
// segment B); int4 loads when both segments are 16-byte aligned multiples of 4
// Column window (colF > 0): the id stream is a [n / colF][colF] matrix and only columns c0 .. c0+nc-1 can hold rows
// of this workgroup's range (DLRM: column f of the combined-table ids only holds rows of table f) -- the others
// are not read at all.
template <class F>
__device__ __forceinline__ void for_each_ref(const int32_t* idsA, int64_t nA, const int32_t* idsB, int64_t n, bool vec, F f,
                                             int colF = 0, int c0 = 0, int nc = 0) {
    if (colF > 0) {
        const int64_t m = (n / colF) * nc;
        for (int64_t t = threadIdx.x; t < m; t += DD_THREADS) {
            const int64_t r = t / nc;
            const int64_t j = r * colF + c0 + (t - r * nc);
            f(j, idsA[j]);
        }
        return;
    }
    if (vec) {
        // four independent 16-byte loads in flight per thread: the scan is latency-bound otherwise
        const int64_t n4 = n >> 2, nA4 = nA >> 2;
        for (int64_t q0 = threadIdx.x; q0 < n4; q0 += 4 * DD_THREADS) {
            int4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t q = q0 + (int64_t)k * DD_THREADS;
                if (q < n4) v[k] = q < nA4 ? reinterpret_cast<const int4*>(idsA)[q] : reinterpret_cast<const int4*>(idsB)[q - nA4];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t q = q0 + (int64_t)k * DD_THREADS;
                if (q < n4) { f(4 * q + 0, v[k].x); f(4 * q + 1, v[k].y); f(4 * q + 2, v[k].z); f(4 * q + 3, v[k].w); }
            }
        }
    } else {
        for (int64_t j = threadIdx.x; j < n; j += DD_THREADS) f(j, j < nA ? idsA[j] : idsB[j - nA]);
    }
}

// exclusive prefix sum of one int per thread over the DD_THREADS-thread workgroup; `total` = sum
__device__ __forceinline__ int block_scan_excl(int v, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < DD_THREADS / 64; ++k) {
        const int t = wave_tot[k];
        if (k < wave) before += t;
        all += t;
    }
    __syncthreads();            // wave_tot may be reused
    total = all;
    return before + incl - v;
}

__device__ __forceinline__ unsigned int lds_peek(const unsigned int* p) { return *reinterpret_cast<const volatile unsigned int*>(p); }
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- staging ------------------------------------------------------------------------------
// Rows referenced >= 3 times in a step ("tri" rows: hot items of a skewed id distribution) do not
// take atomics: every such reference gets a private slot in a staging buffer, the slots of a row
// are contiguous, and whoever applies the row sums its segment.  The plan is made here, on the
// id arrays alone:
//   dense numbering of the bucket's tri rows (popcount prefix over the tri bitmap, kept where the
//   "seen" bitmap lived), a per-step allocator hands the bucket a range of dense numbers;
//   in pass 2 every tri reference takes rank = atomicAdd(count[dense], 1) and records
//   (dense, rank); after the pass the counts are final: a second scan gives every row its
//   segment start.  A reference's slot = segstart[dense] + rank (computed by the fused kernel).
// The duplicate list carries (segment start, count) per row.  A segment longer than ORX_SEG_DIRECT
// is reduced by a tree of 64-to-1 partial sums before the apply (hot_reduce_kernel, up to three
// levels, plain stores only: same-address fp32 atomics cost ~100 ns each on this part, so even
// 200 of them on a hot row would dominate the step); its list entry then points at the last
// level's partial sums (count stored negative).
__global__ __launch_bounds__(DD_THREADS) void dedup_kernel(DedupArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned int dd_lds[];
    unsigned int* seen = dd_lds;
    unsigned int* dup = dd_lds + DD_WORDS;
    unsigned int* tri = dd_lds + 2 * DD_WORDS;
    __shared__ int list_base;
    __shared__ int list_cnt;
    __shared__ int wave_tot[DD_THREADS / 64];
    __shared__ int sh_dense, sh_seg, sh_late;
    const int per_step = a.nbu + a.nbi;
    const int64_t s = blockIdx.x / per_step;
    int bk = blockIdx.x % per_step;
    const bool is_user = bk < a.nbu;
    if (!is_user) bk -= a.nbu;
    const int64_t r0 = (int64_t)bk * DD_ROWS;
    const int64_t rows = is_user ? a.NU : a.NI;
    const int64_t nA = is_user ? a.nU : a.nP;                // length of the first id segment
    const int32_t* idsA = (is_user ? a.uid : a.pid) + s * a.id_stride;
    const int32_t* idsB = a.nid + s * a.id_stride;
    const int64_t n = is_user ? a.nU : a.nP + a.nN;
    const int64_t ref0 = is_user ? 0 : a.nU;
    unsigned char* dflag = a.dflag ? a.dflag + s * a.flag_stride : nullptr;
    int32_t* ids_out = a.ids_out ? a.ids_out + s * a.flag_stride : nullptr;
    unsigned char* roles = a.roles ? a.roles + s * a.flag_stride : nullptr;
    // position of reference j in ids_out: [role][role_stride] (role 0 user, 1 pos item, 2 neg item)
    auto out_index = [&](int64_t j) -> int64_t {
        if (a.role_stride == 0) return ref0 + j;
        if (is_user) return j;
        return j < nA ? a.role_stride + j : 2 * a.role_stride + (j - nA);
    };
    const bool vec = ((nA & 3) == 0) && ((n & 3) == 0) && ((((uintptr_t)idsA) | ((uintptr_t)idsB)) & 15) == 0;

    for (int i = threadIdx.x; i < 3 * DD_WORDS; i += DD_THREADS) dd_lds[i] = 0u;
    if (threadIdx.x == 0) { list_cnt = 0; sh_late = 0; }
    __syncthreads();
    int late = 0;                                            // third-or-later references seen by this thread
    const int colF = (!is_user && a.col_win != nullptr) ? a.col_F : 0;
    const int2 cwin = colF ? a.col_win[bk] : make_int2(0, 0);   // (first column, number of columns) of this range
    for_each_ref(idsA, nA, idsB, n, vec, [&](int64_t j, int id) {
        const int64_t l = (int64_t)id - r0;
        if ((uint64_t)l < (uint64_t)DD_ROWS && id_ok(id, rows)) {
            const unsigned int bit = 1u << (l & 31);
            // The bitmaps only ever gain bits: a plain read that already shows the bit decides like the atomic would, and
            // only references that still see it clear go through the atomic (which arbitrates exactly one "first" and one
            // "second").  Thousands of references to ONE row (a 3-row DLRM table, the head of a Zipf distribution) would
            // otherwise serialize three LDS atomics each on the same word (Zipf(1.05) items at C2: 53.7 -> 50.7 us/step).
            const unsigned int cur = lds_peek(&seen[l >> 5]);
            const unsigned int old = (cur & bit) ? cur : atomicOr(&seen[l >> 5], bit);
            int role = 0;                                    // 0: first reference of the row, 1: second, 2: later
            if (old & bit) {
                const unsigned int cur2 = lds_peek(&dup[l >> 5]);
                const unsigned int old2 = (cur2 & bit) ? cur2 : atomicOr(&dup[l >> 5], bit);
                role = 1;
                if (old2 & bit) {
                    if (!(lds_peek(&tri[l >> 5]) & bit)) atomicOr(&tri[l >> 5], bit);
                    role = 2; ++late;
                }
            }
            if (roles) roles[out_index(j)] = (unsigned char)role;
            if (a.first_only) dflag[ref0 + j] = (old & bit) ? 1 : 0;
        }
    }, colF, cwin.x, cwin.y);
    if (a.refinfo != nullptr && late) atomicAdd(&sh_late, late);
    if (a.first_only) return;
    __syncthreads();
    // staging plan, part 1: dense numbers for the tri rows of this range
    int* prefix = reinterpret_cast<int*>(seen);             // "seen" is dead after pass 1
    // up to DD_WORDS/2 tri rows: 16-bit prefixes in the first half of that space, the rows' reference
    // counters in the second half (LDS atomics instead of global ones: a hot row takes thousands)
    unsigned short* prefix16 = reinterpret_cast<unsigned short*>(seen);
    int* lcnt = reinterpret_cast<int*>(seen) + DD_WORDS / 2;
    bool lds_cnt = false;
    int ntri = 0;                                            // tri rows of the range (workgroup-uniform)
    int dense0 = 0;
    int2* refinfo = nullptr; int* tricnt = nullptr; int* segstart = nullptr;
    // the plan pays for itself only where atomics would pile up: ranges with at least max(64, n/512)
    // third-or-later references (uniform ids over a large table stay below: ~110 per range at the
    // headline sizes); elsewhere role-2 references keep atomics, marked by refinfo = (-1, 0)
    const bool plan = a.refinfo != nullptr && sh_late >= (n / 512 > 64 ? n / 512 : 64);
    if (a.refinfo != nullptr) refinfo = a.refinfo + s * a.flag_stride;
    if (plan) {
        tricnt = a.tricnt + s * a.tri_stride; segstart = a.segstart + s * a.tri_stride;
        int mine3 = 0;
        for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) mine3 += __popc(tri[w]);
        int run = block_scan_excl(mine3, wave_tot, ntri);
        if (ntri) {
            if (threadIdx.x == 0) sh_dense = atomicAdd(a.alloc + 8 * s, ntri);
            lds_cnt = ntri <= DD_WORDS / 2;
            if (lds_cnt) {
                for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) { prefix16[w] = (unsigned short)run; run += __popc(tri[w]); }
                for (int i = threadIdx.x; i < ntri; i += DD_THREADS) lcnt[i] = 0;
            } else {
                for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) { prefix[w] = run; run += __popc(tri[w]); }
            }
            __syncthreads();
            dense0 = sh_dense;
        }
    }
    for_each_ref(idsA, nA, idsB, n, vec, [&](int64_t j, int id) {
        const int64_t l = (int64_t)id - r0;
        const bool ok = id_ok(id, rows);
        if ((uint64_t)l < (uint64_t)DD_ROWS && ok) {
            const unsigned int d = (dup[l >> 5] >> (l & 31)) & 1u;
            if (dflag) dflag[ref0 + j] = (unsigned char)d;
            if (ids_out) {
                uint32_t v = (uint32_t)id | (d << 31);
                if (roles && d) {
                    // rows with exactly two references: one plain store each into two scratch rows;
                    // three or more: every reference uses atomics (role 2)
                    const unsigned int tw = tri[l >> 5];
                    const unsigned int t3 = (tw >> (l & 31)) & 1u;
                    v |= (t3 ? 2u : (uint32_t)roles[out_index(j)]) << 29;
                    if (t3 && ntri) {
                        const int d = (lds_cnt ? (int)prefix16[l >> 5] : prefix[l >> 5]) + __popc(tw & ((1u << (l & 31)) - 1u));
                        refinfo[out_index(j)] = make_int2(dense0 + d, lds_cnt ? atomicAdd(lcnt + d, 1) : atomicAdd(tricnt + dense0 + d, 1));
                    } else if (t3 && refinfo != nullptr) {
                        refinfo[out_index(j)] = make_int2(-1, 0);
                    }
                }
                ids_out[out_index(j)] = (int32_t)v;
            }
        } else if (!ok && bk == 0 && ids_out) {
            ids_out[out_index(j)] = 0x7fffffff;              // out-of-range id: can never be a valid row
        }
    }, colF, cwin.x, cwin.y);
    if (a.dupbits != nullptr) {      // keep the "seen twice" bitmap of (step, range) for urgent_kernel
        unsigned int* out = a.dupbits + ((size_t)s * per_step + (is_user ? bk : a.nbu + bk)) * DD_WORDS;
        for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) out[w] = dup[w];
    }
    // staging plan, part 2: the counts are final -> segment start of every tri row.  A thread's tri rows
    // are numbered q = 0, 1, ... in (word, bit) order; count and segment start of the first TQ stay in
    // registers for the list emission below (one global round trip instead of three).
    constexpr int TQ = 6;
    int qcnt[TQ], qseg[TQ];
    // constant-index access only (a dynamically indexed local array would live in scratch memory)
    auto qput = [](int (&arr)[TQ], int q, int v) {
#pragma unroll
        for (int i = 0; i < TQ; ++i) if (q == i) arr[i] = v;
    };
    auto qget = [](const int (&arr)[TQ], int q) {
        int v = 0;
#pragma unroll
        for (int i = 0; i < TQ; ++i) if (q == i) v = arr[i];
        return v;
    };
    if (ntri) {
        // counts of this range are only ever touched by this workgroup (atomics and agent-scope loads at
        // the same L2): the barrier orders them, no fence (an agent-scope release writes back the whole L2)
        __syncthreads();
        int csum = 0, q = 0;
        for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) {
            const int c = __popc(tri[w]);
            const int d0 = lds_cnt ? (int)prefix16[w] : prefix[w];
            for (int k = 0; k < c; ++k, ++q) {
                const int v = lds_cnt ? lcnt[d0 + k] : ld_agent(tricnt + dense0 + d0 + k);
                qput(qcnt, q, v);
                csum += v;
            }
        }
        int total_refs;
        int run = block_scan_excl(csum, wave_tot, total_refs);
        if (threadIdx.x == 0) sh_seg = atomicAdd(a.alloc + 8 * s + 1, total_refs);
        __syncthreads();
        run += sh_seg;
        q = 0;
        for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) {
            const int c = __popc(tri[w]);
            const int d0 = lds_cnt ? (int)prefix16[w] : prefix[w];
            for (int k = 0; k < c; ++k, ++q) {
                segstart[dense0 + d0 + k] = run;
                qput(qseg, q, run);
                run += q < TQ ? qget(qcnt, q) : (lds_cnt ? lcnt[d0 + k] : ld_agent(tricnt + dense0 + d0 + k));
            }
        }
    }
    // append the duplicated rows of this range to the step's list
    int mine = 0;
    for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) mine += __popc(dup[w]);
    int off = 0;
    if (mine) off = atomicAdd(&list_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) list_base = list_cnt ? atomicAdd(a.dcount + s, list_cnt) : 0;
    __syncthreads();
    if (mine) {
        int64_t e = s * a.list_stride + list_base + off;
        const uint32_t tag = is_user ? 0u : 0x80000000u;
        int q = 0;
        for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) {
            unsigned int m = dup[w];
            const unsigned int tw = tri[w];
            while (m) {
                const int bpos = __ffs(m) - 1;
                m &= m - 1;
                const uint32_t ent = (uint32_t)(r0 + (int64_t)w * 32 + bpos) | tag;
                a.dlist[e] = ent;
                if (a.dcnt != nullptr) {
                    int c = 0, sg = 0;
                    if (ntri && ((tw >> bpos) & 1u)) {      // this thread wrote segstart[dense] itself (same word)
                        if (q < TQ) { c = qget(qcnt, q); sg = qget(qseg, q); }
                        else {
                            const int d = (lds_cnt ? (int)prefix16[w] : prefix[w]) + __popc(tw & ((1u << bpos) - 1u));
                            c = lds_cnt ? lcnt[d] : ld_agent(tricnt + dense0 + d);
                            sg = segstart[dense0 + d];
                        }
                        ++q;
                        if (c > ORX_SEG_DIRECT) {           // long segment: reduction tree
                            int4* items = a.items + s * a.item_stride;
                            int src = sg, len = c, level = 0;
                            do {
                                const int pieces = (len + ORX_PIECE - 1) / ORX_PIECE;
                                const int b0 = a.tree_off[level] + atomicAdd(a.alloc + 8 * s + 2 + level, pieces);
                                for (int k = 0; k < pieces; ++k) {
                                    const int rem = len - k * ORX_PIECE;
                                    items[b0 + k] = make_int4(src + k * ORX_PIECE, rem < ORX_PIECE ? rem : ORX_PIECE, b0 + k, 0);
                                }
                                src = b0; len = pieces; ++level;
                            } while (len > ORX_SEG_DIRECT && level < 3);
                            sg = src; c = -len;
                        }
                    }
                    a.dseg[e] = sg; a.dcnt[e] = c;
                }
                ++e;
            }
        }
    }
}

int orx_dedup_buckets(int64_t rows) { return (int)((rows + DD_ROWS - 1) / DD_ROWS); }
int64_t orx_dedup_range_rows() { return DD_ROWS; }
int orx_dedup_words(void) { return DD_WORDS; }

int orx_launch_dedup(orx_ctx* ctx, const DedupArgs& a, int64_t K) {
    ProfScope ps(ctx, ORX_K_DEDUP);
    const int64_t g = K * (a.nbu + a.nbi);
    if (g == 0) return ORX_OK;
    ORX_ARG(g < (1LL << 31), "dedup: grid too large (K=%lld, buckets=%d)", (long long)K, a.nbu + a.nbi);
    ORX_ONCE_PER_DEVICE(ctx, ORX_HIP(hipFuncSetAttribute((const void*)dedup_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, DD_LDS_BYTES)));
    ORX_LAUNCH(ctx, dedup_kernel, dim3((unsigned)g), dim3(DD_THREADS), DD_LDS_BYTES, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// A reference of step s whose row was duplicated in step s-1 is "urgent": the row's update of step
// s-1 is applied by the apply blocks of the SAME launch that processes step s (see fused_kernel),
// so this reference has to wait for the row's ready flag.  Marks such references with bit 28.
__global__ __launch_bounds__(DD_THREADS) void urgent_kernel(DedupArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned int dd_lds[];
    const int per_step = a.nbu + a.nbi;
    const int64_t s = 1 + blockIdx.x / per_step;             // steps 1 .. K-1 of the chunk
    int bk = blockIdx.x % per_step;
    const unsigned int* prev = a.dupbits + ((size_t)(s - 1) * per_step + bk) * DD_WORDS;
    const bool is_user = bk < a.nbu;
    if (!is_user) bk -= a.nbu;
    const int64_t r0 = (int64_t)bk * DD_ROWS;
    const int64_t rows = is_user ? a.NU : a.NI;
    const int64_t nA = is_user ? a.nU : a.nP;
    const int32_t* idsA = (is_user ? a.uid : a.pid) + s * a.id_stride;
    const int32_t* idsB = a.nid + s * a.id_stride;
    const int64_t n = is_user ? a.nU : a.nP + a.nN;
    int32_t* ids_out = a.ids_out + s * a.flag_stride;
    const bool vec = ((nA & 3) == 0) && ((n & 3) == 0) && ((((uintptr_t)idsA) | ((uintptr_t)idsB)) & 15) == 0;
    for (int w = threadIdx.x; w < DD_WORDS; w += DD_THREADS) dd_lds[w] = prev[w];
    __syncthreads();
    for_each_ref(idsA, nA, idsB, n, vec, [&](int64_t j, int id) {
        const int64_t l = (int64_t)id - r0;
        if ((uint64_t)l < (uint64_t)DD_ROWS && id_ok(id, rows) && ((dd_lds[l >> 5] >> (l & 31)) & 1u)) {
            const int64_t idx = is_user ? j : (j < nA ? a.role_stride + j : 2 * a.role_stride + (j - nA));
            ids_out[idx] |= (1 << 28);
        }
    });
}

int orx_launch_urgent(orx_ctx* ctx, const DedupArgs& a, int64_t K) {
    ProfScope ps(ctx, ORX_K_DEDUP);
    const int64_t g = (K - 1) * (a.nbu + a.nbi);
    if (g <= 0) return ORX_OK;
    ORX_LAUNCH(ctx, urgent_kernel, dim3((unsigned)g), dim3(DD_THREADS), DD_WORDS * 4, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// -------------------------------------------------- loss partial reduction ---
// One block per step: sum nwaves x {loss, l2} fp32 partials in fp64.
__device__ __forceinline__ void loss_reduce_body(const ReduceArgs& a, int step) {
    __shared__ double sh[2][16];
    const float* part = a.partial + (size_t)step * a.nwaves * 2;
    double s0 = 0.0, s1 = 0.0;
    constexpr int UN = 8;                                    // 8 independent loads in flight per thread (the pass is latency-bound)
    for (int i0 = threadIdx.x; i0 < a.nwaves; i0 += UN * blockDim.x) {
        float2 v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = i0 + u * blockDim.x;
            v[u] = i < a.nwaves ? *reinterpret_cast<const float2*>(part + 2 * i) : make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) { s0 += (double)v[u].x; s1 += (double)v[u].y; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh[0][w] = s0; sh[1][w] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { t0 += sh[0][k]; t1 += sh[1][k]; }
        a.out[2 * step] = t0;
        a.out[2 * step + 1] = t1;
    }
}

__global__ __launch_bounds__(1024) void loss_reduce_kernel(ReduceArgs a) { loss_reduce_body(a, (int)blockIdx.x); }

int orx_launch_loss_reduce(orx_ctx* ctx, const ReduceArgs& a, int64_t K) {
    ProfScope ps(ctx, ORX_K_REDUCE);
    ORX_LAUNCH(ctx, loss_reduce_kernel, dim3((unsigned)K), dim3(1024), 0, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// fused_kernel / fused_generic_kernel and their launch dispatch: orx_fused_device.h (shared with kernels_pairwise_weighted.hip)
#include "orx_fused_device.h"

// dup_apply: one group of LPR lanes per duplicated row of the step.
template <int LPR, int OPT>
__device__ __forceinline__ void dup_apply_body(const PairArgs& a, int block, int nblocks) {
    constexpr int TPW = 64 / LPR;
    constexpr int D = 4 * LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int n = *a.dcount;
    const int wpb = (int)(blockDim.x >> 6);             // wavefronts per block (256 or 1024 threads)
    const int64_t stride = (int64_t)nblocks * wpb * TPW;
    for (int64_t e = ((int64_t)block * wpb + (threadIdx.x >> 6)) * TPW + grp; e < n; e += stride) {
        const uint32_t ent = a.dlist[e];
        if (ent == ORX_DLIST_DEAD) continue;            // (the row was paired after all: updated in place by the step's launch)
        const bool item = (ent >> 31) != 0;
        const size_t row = ent & 0x7fffffffu;
        float* W = item ? a.V : a.U;
        float* G = item ? a.gV : a.gU;
        float* A = item ? a.aV : a.aU;
        float* G2 = item ? a.gV2 : a.gU2;
        float* gp = G + row * D + 4 * sub;
        float* wp = W + row * D + 4 * sub;
        // staged row: scnt > 0: sum its staging segment here; scnt < 0: hot_reduce_kernel has reduced the
        // (long) segment to -scnt partial sums; scnt == 0: two-reference row, scratch rows
        const int scnt = a.dcnt != nullptr ? a.dcnt[e] : 0;
        const int sseg = scnt != 0 ? a.dseg[e] : 0;
        const f4 w = *reinterpret_cast<const f4*>(wp);
        f4 z; z.x = z.y = z.z = z.w = 0.0f;
        f4 g;
        if (scnt > 0) {
            g = segment_sum4<D>(a.stage, sseg, scnt, sub);
        } else if (scnt < 0) {
            g = segment_sum4<D>(a.part, sseg, -scnt, sub);
        } else {
            g = *reinterpret_cast<const f4*>(gp);
            *reinterpret_cast<f4*>(gp) = z;
            if (G2 != nullptr) {
                g = g + *reinterpret_cast<const f4*>(G2 + row * D + 4 * sub);
                *reinterpret_cast<f4*>(G2 + row * D + 4 * sub) = z;
            }
        }
        if (OPT == ORX_ADAM) {
            float* A2 = item ? a.a2V : a.a2U;
            int* L = item ? a.lastV : a.lastU;
            f4 wn = w;
            f4 mm = *reinterpret_cast<const f4*>(A + row * D + 4 * sub), vv = *reinterpret_cast<const f4*>(A2 + row * D + 4 * sub);
            adam_catchup4(wn, mm, vv, L[row], a.step_t - 1, a.lrt, a.b1, a.b2, a.eps);
            adam_elem4(wn, mm, vv, g, a.lrt[a.step_t], a.b1, a.b2, a.eps);
            if (a.censor) {
                wn = censor4<LPR>(wn, a.min_norm);
                if (item && censored_twice(a, row, a.epoch)) wn = censor4<LPR>(wn, a.min_norm);
            }
            *reinterpret_cast<f4*>(wp) = wn; *reinterpret_cast<f4*>(A + row * D + 4 * sub) = mm; *reinterpret_cast<f4*>(A2 + row * D + 4 * sub) = vv;
            if (sub == 0) L[row] = a.step_t;
        } else if (a.censor) {
            f4 wn = censor4<LPR>(opt_new4<OPT>(A + row * D + 4 * sub, w, g, a.lr, a.eps), a.min_norm);
            if (item && censored_twice(a, row, a.epoch)) wn = censor4<LPR>(wn, a.min_norm);
            *reinterpret_cast<f4*>(wp) = wn;
        } else {
            opt_apply4<OPT>(wp, A + row * D + 4 * sub, w, g, a.lr, a.eps);
        }
        float gbs = 0.0f;
        if (scnt != 0 && item && a.b != nullptr)
            gbs = scnt > 0 ? segment_sum1<LPR>(a.stageb, sseg, scnt, sub) : segment_sum1<LPR>(a.partb, sseg, -scnt, sub);
        if (item && a.b != nullptr && sub == 0) {
            float gb = gbs;
            if (scnt == 0) {
                gb = a.gb[row];
                a.gb[row] = 0.0f;
                if (a.gb2 != nullptr) { gb += a.gb2[row]; a.gb2[row] = 0.0f; }
            }
            if (OPT == ORX_ADAM) {
                float bw = a.b[row], bm = a.ab[row], bv = a.a2b[row];
                adam_catchup1(bw, bm, bv, a.lastb[row], a.step_t - 1, a.lrt, a.b1, a.b2, a.eps);
                adam_elem(bw, bm, bv, gb, a.lrt[a.step_t], a.b1, a.b2, a.eps);
                a.b[row] = bw; a.ab[row] = bm; a.a2b[row] = bv; a.lastb[row] = a.step_t;
            } else {
                opt_apply1<OPT>(a.b + row, a.ab + row, a.b[row], gb, a.lr, a.eps);
            }
        }
    }
}

template <int LPR, int OPT>
__global__ __launch_bounds__(256) void dup_apply_kernel(PairArgs a) { dup_apply_body<LPR, OPT>(a, (int)blockIdx.x, (int)gridDim.x); }

// The tail of a K-step call in ONE launch: the duplicated rows of the last step (what dup_apply_kernel does) and, in the first
// `nred` blocks, the per-step sums of the loss partials (what loss_reduce_kernel does) -- two launches and the gap between them
// fewer at the end of every call.
template <int LPR, int OPT>
__global__ __launch_bounds__(1024) void tail_kernel(PairArgs a, ReduceArgs r, int nred) {
    if ((int)blockIdx.x < nred) { loss_reduce_body(r, (int)blockIdx.x); return; }
    dup_apply_body<LPR, OPT>(a, (int)blockIdx.x - nred, (int)gridDim.x - nred);
}

// hot_reduce: one level of the reduction tree over long staging segments.  One wavefront per work
// item (src, len <= ORX_PIECE, dst): its 64/LPR lane groups each sum every (64/LPR)-th vector, the
// groups combine by cross-lane shuffles and group 0 stores the partial sum.  Level 1 reads the
// staged gradients, levels 2 and 3 the partial sums of the level below.  No atomics.
template <int LPR>
__global__ __launch_bounds__(256) void hot_reduce_kernel(PairArgs a, int level) {
    constexpr int TPW = 64 / LPR;
    constexpr int D = 4 * LPR;
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR;
    const int grp = lane / LPR;
    const int n = a.nitems[level];
    const int4* items = a.items + a.tree_off[level];
    const float* src = level == 0 ? a.stage : a.part;
    const float* srcb = level == 0 ? a.stageb : a.partb;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += stride) {
        const int4 it = items[c];
        const float* p = src + (size_t)it.x * D + 4 * sub;
        f4 s0, s1; s0.x = s0.y = s0.z = s0.w = 0.0f; s1 = s0;
        int k = grp;
        for (; k + 3 * TPW < it.y; k += 4 * TPW) {
            const f4 a0 = *reinterpret_cast<const f4*>(p + (size_t)(k + 0 * TPW) * D);
            const f4 a1 = *reinterpret_cast<const f4*>(p + (size_t)(k + 1 * TPW) * D);
            const f4 a2 = *reinterpret_cast<const f4*>(p + (size_t)(k + 2 * TPW) * D);
            const f4 a3 = *reinterpret_cast<const f4*>(p + (size_t)(k + 3 * TPW) * D);
            s0 = s0 + (a0 + a1); s1 = s1 + (a2 + a3);
        }
        for (; k < it.y; k += TPW) s0 = s0 + *reinterpret_cast<const f4*>(p + (size_t)k * D);
        f4 g = s0 + s1;
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            g.x += __shfl_xor(g.x, off); g.y += __shfl_xor(g.y, off); g.z += __shfl_xor(g.z, off); g.w += __shfl_xor(g.w, off);
        }
        if (grp == 0) *reinterpret_cast<f4*>(a.part + (size_t)it.z * D + 4 * sub) = g;
        if (a.b != nullptr) {
            const float gb = wave_sum(lane < it.y ? srcb[it.x + lane] : 0.0f);
            if (lane == 0) a.partb[it.z] = gb;
        }
    }
}

template <int OPT>
__global__ __launch_bounds__(256) void dup_apply_generic_kernel(PairArgs a) {
    const int lane = threadIdx.x & 63;
    const int D = a.D;
    const int n = *a.dcount;
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += stride) {
        const uint32_t ent = a.dlist[e];
        const bool item = (ent >> 31) != 0;
        const size_t row = ent & 0x7fffffffu;
        float* W = item ? a.V : a.U;
        float* G = item ? a.gV : a.gU;
        float* A = item ? a.aV : a.aU;
        float* G2 = item ? a.gV2 : a.gU2;
        for (int k = lane; k < D; k += 64) {
            const size_t i = row * D + k;
            float g = G[i];
            G[i] = 0.0f;
            if (G2 != nullptr) { g += G2[i]; G2[i] = 0.0f; }
            opt_apply1<OPT>(W + i, A + i, W[i], g, a.lr, a.eps);
        }
        if (item && a.b != nullptr && lane == 0) {
            float gb = a.gb[row];
            a.gb[row] = 0.0f;
            if (a.gb2 != nullptr) { gb += a.gb2[row]; a.gb2[row] = 0.0f; }
            opt_apply1<OPT>(a.b + row, a.ab + row, a.b[row], gb, a.lr, a.eps);
        }
    }
}

// ---------------------------------------------------------------- launchers ---
int orx_fused_nwaves(int D, int64_t B) { return (int)(fused_grid(D, B) * 4); }

int orx_fused_can_inline_apply(int D) { return lpr_for_dim(D) != 0; }
int orx_fused_tpw(int D) { const int lpr = lpr_for_dim(D); return lpr ? 64 / lpr : 0; }

int orx_launch_fused(orx_ctx* ctx, int model, int optkind, int mode, const PairArgs& a) {
    if (a.wt != nullptr) return orx_launch_fused_weighted(ctx, model, optkind, mode, a);      // (its instantiations: kernels_pairwise_weighted.hip)
    return launch_fused_any<false>(ctx, model, optkind, mode, a);
}

template <int OPT>
static void launch_dup_apply_lpr(int lpr, dim3 g, orx_ctx* s, const PairArgs& a) {
    switch (lpr) {
        case 4: ORX_LAUNCH(s, (dup_apply_kernel<4, OPT>), g, dim3(256), 0, a); break;
        case 8: ORX_LAUNCH(s, (dup_apply_kernel<8, OPT>), g, dim3(256), 0, a); break;
        case 16: ORX_LAUNCH(s, (dup_apply_kernel<16, OPT>), g, dim3(256), 0, a); break;
        case 32: ORX_LAUNCH(s, (dup_apply_kernel<32, OPT>), g, dim3(256), 0, a); break;
        case 64: ORX_LAUNCH(s, (dup_apply_kernel<64, OPT>), g, dim3(256), 0, a); break;
        default: ORX_LAUNCH(s, (dup_apply_generic_kernel<OPT>), g, dim3(256), 0, a); break;
    }
}

int orx_launch_hot_reduce(orx_ctx* ctx, const PairArgs& a, int level) {
    ProfScope ps(ctx, ORX_K_DUPAPPLY);
    const int lpr = lpr_for_dim(a.D);
    const dim3 g(level == 0 ? 2048 : 256);
    switch (lpr) {
        case 4: ORX_LAUNCH(ctx, (hot_reduce_kernel<4>), g, dim3(256), 0, a, level); break;
        case 8: ORX_LAUNCH(ctx, (hot_reduce_kernel<8>), g, dim3(256), 0, a, level); break;
        case 16: ORX_LAUNCH(ctx, (hot_reduce_kernel<16>), g, dim3(256), 0, a, level); break;
        case 32: ORX_LAUNCH(ctx, (hot_reduce_kernel<32>), g, dim3(256), 0, a, level); break;
        case 64: ORX_LAUNCH(ctx, (hot_reduce_kernel<64>), g, dim3(256), 0, a, level); break;
        default: orx_set_error("hot_reduce: no staging for dim %d", a.D); return ORX_ERR_ARG;
    }
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}

// dup_apply of the call's last step + loss_reduce of its K steps in one launch (float4 dims; SGD / Adagrad); false: not applicable
bool orx_launch_tail(orx_ctx* ctx, int optkind, const PairArgs& a, const ReduceArgs& r, int64_t K, int* rc) {
    const int lpr = lpr_for_dim(a.D);
    if (lpr == 0 || optkind == ORX_ADAM || K > 4096) return false;
    ProfScope ps(ctx, ORX_K_DUPAPPLY);
    int64_t want = (a.B * 3 / 16) / (16 * (64 / lpr)) + 1;      // (1024-thread blocks: the loss sums want them)
    if (want > 512) want = 512;
    if (want < 16) want = 16;
    const dim3 g((unsigned)(want + K));
#define ORX_TL(L) do { if (optkind == ORX_ADAGRAD) ORX_LAUNCH(ctx, (tail_kernel<L, ORX_ADAGRAD>), g, dim3(1024), 0, a, r, (int)K); \
                       else if (optkind == ORX_MOMENTUM) ORX_LAUNCH(ctx, (tail_kernel<L, ORX_MOMENTUM>), g, dim3(1024), 0, a, r, (int)K); \
                       else ORX_LAUNCH(ctx, (tail_kernel<L, ORX_SGD>), g, dim3(1024), 0, a, r, (int)K); } while (0)
    switch (lpr) {
        case 4: ORX_TL(4); break;
        case 8: ORX_TL(8); break;
        case 16: ORX_TL(16); break;
        case 32: ORX_TL(32); break;
        default: ORX_TL(64); break;
    }
#undef ORX_TL
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { orx_set_error("tail_kernel launch failed: %s", hipGetErrorString(e)); *rc = ORX_ERR_HIP; } else *rc = ORX_OK;
    return true;
}

// The number of duplicated rows lives in device memory: fixed grid, grid-stride loop.
int orx_launch_dup_apply(orx_ctx* ctx, int optkind, const PairArgs& a) {
    ProfScope ps(ctx, ORX_K_DUPAPPLY);
    const int lpr = lpr_for_dim(a.D);
    int64_t want = (a.B * 3 / 16) / (lpr ? 4 * (64 / lpr) : 4) + 1;     // ~ expected duplicates of a uniform batch
    if (want > 2048) want = 2048;
    if (want < 64) want = 64;
    const dim3 g((unsigned)want);
    if (optkind == ORX_ADAM && a.lrt != nullptr && lpr != 0) {       // lazy Adam (never the generic-dim kernel)
        switch (lpr) {
            case 4: ORX_LAUNCH(ctx, (dup_apply_kernel<4, ORX_ADAM>), g, dim3(256), 0, a); break;
            case 8: ORX_LAUNCH(ctx, (dup_apply_kernel<8, ORX_ADAM>), g, dim3(256), 0, a); break;
            case 16: ORX_LAUNCH(ctx, (dup_apply_kernel<16, ORX_ADAM>), g, dim3(256), 0, a); break;
            case 32: ORX_LAUNCH(ctx, (dup_apply_kernel<32, ORX_ADAM>), g, dim3(256), 0, a); break;
            default: ORX_LAUNCH(ctx, (dup_apply_kernel<64, ORX_ADAM>), g, dim3(256), 0, a); break;
        }
    } else if (optkind == ORX_ADAGRAD) launch_dup_apply_lpr<ORX_ADAGRAD>(lpr, g, ctx, a);
    else if (optkind == ORX_MOMENTUM) launch_dup_apply_lpr<ORX_MOMENTUM>(lpr, g, ctx, a);
    else launch_dup_apply_lpr<ORX_SGD>(lpr, g, ctx, a);
    ORX_HIP(hipGetLastError());
    return ORX_OK;
}
