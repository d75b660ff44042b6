// Posterior variance + acquisition + arg-max, fused.
//
// Replaces, for every candidate c,
//     Sigma = K** - K*x inv K*x^T ; cov_func = sqrt(|diag Sigma|)        point_selector.py:91,98
//     acq   = explore * cov_func - mean_func ; argwhere(acq == amax)[0]   point_selector.py:204,207
// The reference forms the full M x M matrix; only its diagonal is ever used, and
//     diag_c = prior_var - |v_c|^2,   v_c = L^-1 k_c = U^T k_c,   U = L^-T (upper triangular).
// V = KsT^T * U is a dense triangular product: it runs on v_mfma_f64_16x16x4_f64 and V itself is
// never stored - each 256 x 128 block of V is squared and row-summed out of the accumulators.
//
// Workgroup = 512 threads = 8 waves, owns 256 candidates end to end:
//   for each 128-column block jb of V:   k runs over [0, 128*(jb+1))  (U is upper triangular)
//       16-deep k tiles: KsT tile [16 x 256] and U tile [16 x 128] go global -> LDS directly (LDS-DMA loads,
//       three-stage ring, one barrier in the middle of each k tile), MFMA 4x4 tiles of 16x16 per wave;
//       inside the diagonal block, 16x16 tiles of U that lie wholly below the diagonal are skipped
//   epilogue: row-sum of squares -> sigma -> mean from the per-slice partials -> LCB / EI -> optional
//   dense stores -> block arg-max carrying (value, lowest index).
// Waves w and w+4 share a SIMD; they take the even and the odd 16-column tiles of the block, so that on the
// diagonal (where tiles below U's diagonal are skipped) both always have nearly the same amount of work and
// keep hiding each other's LDS / branch / DMA-issue latencies.
#include "cov_entry.h"
#include "dense_acq.h"

#include <cstdlib>
#include <mutex>
#include <type_traits>

namespace {

constexpr int BM = 256, BN = 128, BK = 16;  // candidates x columns of V per workgroup, k depth of a tile
// Waves per workgroup and their split.  Measured on MI355X (N = 512): 8 waves as 4 x 2 (wave tile 64 x 64, two
// waves per SIMD) run 0.547 ms per 2^17 candidates; 4 waves with 128 x 64 or 64 x 128 wave tiles (one wave per SIMD,
// 256 accumulator registers) run 1.06 / 0.99 ms: hipcc spills 70-100 VGPRs around the tile loop and one wave
// alone does not keep a SIMD's matrix pipe fed across the LDS reads and the barrier; 16 waves (four per SIMD, wave
// tile 32 x 64 or 64 x 32) run 0.560 / 0.594 ms: half again as many LDS fragment reads per MFMA.
#ifndef GPBO_NW
#define GPBO_NW 8
#endif
#ifndef GPBO_WQ
#define GPBO_WQ 2
#endif
constexpr int NW = GPBO_NW;                // waves per workgroup
constexpr int WQ = GPBO_WQ;                // column groups of waves
constexpr int WR = NW / WQ;                // row groups of waves (BM / WR candidates each)
constexpr int MI = BM / WR / 16;           // 16-row tiles per wave
constexpr int NI = BN / WQ / 16;           // 16-column tiles per wave
static_assert(NI % 2 == 0 && (BM % (WR * 16)) == 0, "tile split");
// (measured on MI355X, N = 512: 256 x 128 runs 0.596 ms per 2^17 candidates, 128 x 256 runs 0.635 ms - the
//  wider column block has more k tiles on the diagonal whose MFMA time is shorter than their 48 KB of loads)
constexpr int LDA = BM + 16;  // padded so lanes l and l+16 (k, k+1) of a ds_read_b64 group hit disjoint banks
constexpr int LDB = BN + 16;
constexpr int A_TILE = BK * LDA;
constexpr int B_TILE = BK * LDB;
constexpr int STAGE = A_TILE + B_TILE;

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// 16 bytes per lane, global -> LDS without a VGPR round trip.  The LDS destination is the wave-uniform
// address `l` plus lane*16; the global source is per lane.
// `g` (the tile base) is wave-uniform as well and `off` a 32-bit BYTE offset per lane: the piece is a buffer load through a
// descriptor made of the tile base (buffer_load_dwordx4 v_off, s[desc], 0 offen lds) and needs no vector instruction to form
// a 64-bit address; the global_load_lds form cost one v_lshl_add_u64 per piece, all six into the same register pair.
#ifndef GPBO_SIGMA_STATIC_RING
#define GPBO_SIGMA_STATIC_RING 1  // 0: every k tile through the run-time ring position (A/B builds; see the tile loop)
#endif
#ifndef GPBO_SIGMA_DMA_GLOBAL
#define GPBO_SIGMA_DMA_GLOBAL 0   // 1: the global_load_lds form (A/B builds)
#endif
__device__ __forceinline__ void glds16(const double *g, unsigned off, double *l) {
#if GPBO_SIGMA_DMA_GLOBAL
    __builtin_amdgcn_global_load_lds((glb_void_t *)(reinterpret_cast<const char *>(g) + off), (lds_void_t *)l, 16, 0, 0);
#else
    // raw buffer, stride 0, 2^32 - 1 bytes from the tile base (every offset of a tile is below 2^32: GPBO_CHUNK_MAX, Np <= 2^20)
    const __amdgpu_buffer_rsrc_t desc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(g), 0, -1, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(desc, (lds_void_t *)l, 16, (int)off, 0, 0, 0);
#endif
}

// GRAM (config 5, q = 8 Monte-Carlo qEI): the tiles of V are computed TRANSPOSED (the two operands of every product swapped:
// register r of lane l then holds V[candidate l & 15][column (l >> 4) + 4r] of its tile), which makes one accumulator
// register at once the A operand (row = candidate, k = column) and the B operand (k = column, column = candidate) of
// v_mfma_f64_16x16x4_f64: four products per finished tile add V V^T of its 16 candidates - the joint posterior's Gram
// blocks of two 8-candidate batches - to 8 more accumulators, and V itself never leaves the registers (round 4 wrote the
// 2.1 GB of V per launch for qei_kernel to read back).  `vbuf` then receives the partial Gram blocks:
// [S * WQ partials][ldk / 8 batches][8 x 8].
template <int VARIANT, bool GRAM = false>  // VARIANT 0 = product; others = timing-only diagnostics (GPBO_SIGMA_VARIANT), wrong results
__global__ __launch_bounds__(NW * 64) void sigma_acq_kernel(
    const double *__restrict__ KsT, int64_t ldk, const double *__restrict__ U, int Np,
    const double *__restrict__ mu_part, int nsl, int64_t Mc, double prior_var, int acq_kind, double p0, double p1,
    int64_t idx_base, double *__restrict__ mu_out, double *__restrict__ sigma_out, double *__restrict__ acq_out,
    double *__restrict__ part_val, int64_t *__restrict__ part_idx, unsigned long long *__restrict__ nan_count,
    double *__restrict__ vbuf /* GRAM: the partial Gram blocks of the 8-candidate batches (see above); else unused */,
    double *__restrict__ ss_part /* column-split launches (gridDim.y = S > 1): [S x ldk] partial |v|^2, no epilogue */,
    int xg /* > 1: one-dimensional launch, the xg column groups of a candidate tile 8 linear ids apart (same XCD) */,
    int ntile, int ncb /* > 0: only the first ncb column blocks of V (the prefix-bound screen: |v|^2 over the first
                          128 ncb observations is a LOWER bound of |v|^2, the variance from it an upper bound) */) {
    __shared__ double smem[3 * STAGE];
    // diagnostics: TV = the timing variant (1 = no barrier and no DMA, 2 = no tile skipping on the diagonal, 3 = no barrier,
    // 4 = no DMA, 5 = every fragment read from stage 0, so that the fragment addresses are loop invariants, 7 = as 5 with
    // half of the fragment reads); VARIANT 6 = the product loop with per-tile stamps, 8 + v = timing
    // variant v with per-tile stamps
    constexpr bool STAMP = VARIANT == 6 || VARIANT >= 8;
    constexpr int TV = VARIANT >= 8 ? VARIANT - 8 : (VARIANT == 6 ? 0 : VARIANT);
    // Column split (few candidates, e.g. the re-scoring behind a screen): workgroup (x, s) of S takes the column
    // blocks s, 2S-1-s, 2S+s, 4S-1-s, ... (boustrophedon rounds: block jb costs jb+1 k tiles, so pairing a cheap
    // with an expensive one balances the S workgroups) and leaves its partial row sums for split_finish_kernel.
    int S = (int)gridDim.y, sp = (int)blockIdx.y, tile_x = (int)blockIdx.x;
    if (xg > 1) {
        // Column groups for LARGE launches: with one workgroup per candidate tile, 256 slabs of K*^T (8.4 MB each at
        // N = 4096) are live at a time and every re-read comes from HBM (72 GB per 2^17 candidates, profiles/).  The xg
        // groups of a tile run side by side on one XCD instead (ids 8 apart under the round-robin dispatch - speed only),
        // so 256 / xg slabs are live and the re-reads are served on chip.
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const int q = slot / xg;
        S = xg;
        sp = slot - q * xg;
        tile_x = q * 8 + xcd;
        if (tile_x >= ntile) return;
    }
    auto jb_of = [&](int r) { return r * S + ((r & 1) ? (S - 1 - sp) : sp); };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid % WR, wq = wid / WR;  // SIMD partners w, w+4 get different column groups
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t cand0 = (int64_t)tile_x * BM;

    // staging: global -> LDS directly (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction, no VGPRs).
    // LDS image rows are padded, and every wave instruction's 1 KiB lies inside one row:
    //   A tile (K*^T): 16 rows x BM/128 pieces, B tile (U): 16 rows x BN/128 pieces; wave w takes pieces w + 8r
    // The tile base pointers are wave-uniform and advance incrementally (scalar adds); each lane's share of a
    // piece is a 32-bit element offset fixed for the whole kernel, so one DMA costs a few scalar instructions.
    const double *a_base = KsT + cand0;
    constexpr int AP = BM / 128, BP = BN / 128;  // 1 KiB pieces per row
    constexpr int NPA = BK * AP / NW, NPB = BK * BP / NW;  // 1-KiB pieces per wave per tile
    unsigned voffA[NPA], voffB[NPB];        // byte offsets inside a tile, 8 (row * ld + piece * 128 + lane * 2) < 2^32
    int ldsA[NPA], ldsB[NPB];               // LDS element offsets of the pieces inside a stage
#pragma unroll
    for (int r = 0; r < NPA; ++r) {
        const int u = wid + NW * r, row = u / AP, piece = u % AP;
        voffA[r] = (unsigned)(row * (unsigned)ldk + piece * 128 + lane * 2) * 8u;
        ldsA[r] = row * LDA + piece * 128;
    }
#pragma unroll
    for (int r = 0; r < NPB; ++r) {
        const int u = wid + NW * r, row = u / BP, piece = u % BP;
        voffB[r] = (unsigned)(row * (unsigned)Np + piece * 128 + lane * 2) * 8u;
        ldsB[r] = A_TILE + row * LDB + piece * 128;
    }
    d4_t acc[MI][NI];
    d4_t gram[GRAM ? MI : 1];
#pragma unroll
    for (int i = 0; i < (GRAM ? MI : 1); ++i) gram[i] = d4_t{0.0, 0.0, 0.0, 0.0};
    double ss[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) ss[i][j] = 0.0;
    }

    const int nJ = ncb > 0 ? ncb : Np / BN;
    // staging iterator: tile (pj, pk) goes to stage pbuf; pa / pb are its global bases
    int pr = 0, pj = jb_of(0), pk = 0, pbuf = 0;
    const double *pa = a_base, *pb = U + (int64_t)pj * BN;
    auto stage_next = [&]() {
        double *St = smem + pbuf * STAGE;
#pragma unroll
        for (int r = 0; r < NPA; ++r) glds16(pa, voffA[r], St + ldsA[r]);
#pragma unroll
        for (int r = 0; r < NPB; ++r) glds16(pb, voffB[r], St + ldsB[r]);
        pbuf = (pbuf == 2) ? 0 : pbuf + 1;
        if (++pk == (pj + 1) * (BN / BK)) {  // next column block of this workgroup: k restarts
            pj = jb_of(++pr);
            pk = 0;
            pa = a_base;
            pb = U + (int64_t)pj * BN;
        } else {
            pa += (int64_t)BK * ldk;
            pb += (int64_t)BK * Np;
        }
    };

    // Flattened tile sequence (jb, kt): kt = 0 .. 8(jb+1)-1 for jb = 0 .. nJ-1, three LDS stages.
    // The MFMA stream never stops at a tile boundary: the fragments of the next tile's first step are read
    // during the current tile's last step.  The one barrier per tile sits in the MIDDLE of the tile, where
    // every wave still holds fragments for the following MFMAs in registers, so nobody leaves the barrier
    // into an LDS-latency bubble.  At that barrier (iteration t):
    //   - each wave has first waited for its own LDS-DMA of tile t+1 (issued one tile earlier), so after the
    //     barrier tile t+1 is complete for everyone, half a tile before anyone reads it;
    //   - every wave has left tile t-1, so its stage may be overwritten: the DMA of tile t+2 is issued now.
    stage_next();
    if (pj < nJ) stage_next();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    double a0[MI], b0[NI], a1[MI], b1[NI];
    auto lds_frag = [&](double (&af)[MI], double (&bf)[NI], int buf, int kk) {
        if (TV == 5 || TV == 7) buf = 0;  // timing only: every fragment address is a loop invariant
        const double *As = smem + buf * STAGE;
        const double *Bs = As + A_TILE;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[mi] = As[(kk + l4) * LDA + wr * (BM / WR) + mi * 16 + l15];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) bf[ni] = Bs[(kk + l4) * LDB + (WQ * ni + wq) * 16 + l15];
    };
    lds_frag(a0, b0, 0, 0);
    if (TV == 7) lds_frag(a1, b1, 0, 4);  // timing only: the second fragment set is read here and never again
    int dbg_it = 0;
    int ring = 0;
    // One tile.  FULL = every 16x16 tile of U in it is non-zero (all k tiles left of the diagonal block): the
    // MFMA stream is then free of branches; on the diagonal block, MFMA groups of 16-column tiles that lie wholly
    // below U's diagonal are branched over (wave-uniform).  LDS reads, barrier and DMA are the same in both.
    // RING = the tile's stage where the caller knows it at compile time, -1 = the run-time ring position `ring`.
    auto tile_body = [&](auto full_tag, auto ring_tag, int jb, int kt) {
        constexpr bool FULL = decltype(full_tag)::value;
        constexpr int RING = decltype(ring_tag)::value;
        if (STAMP && vbuf && tid == 0) {  // diagnostic: cycle stamp per tile (timing build only)
            vbuf[(int64_t)blockIdx.x * 1024 + dbg_it] = (double)__builtin_amdgcn_s_memtime();
            if (dbg_it == 0 || (jb == nJ - 1 && kt == nJ * (BN / BK) - 1))  // 100 MHz wall clock at both ends (S = 1)
                vbuf[(int64_t)blockIdx.x * 1024 + (dbg_it == 0 ? 1000 : 1001)] = (double)__builtin_amdgcn_s_memrealtime();
            ++dbg_it;
        }
        const int cur = RING >= 0 ? RING : ring;
        const int nxt = (cur == 2) ? 0 : cur + 1;
        // first 16-column tile of this wave that still has non-zero rows of U in this k tile (>= 4: none)
        // (wave column group wq owns the 16-column tiles WQ ni + wq of the block, so on the diagonal all waves
        //  keep almost the same amount of work: column tile WQ ni + wq is needed iff it is >= kt')
        int ni_min = (kt - jb * (BN / BK) - wq + WQ - 1) / WQ;
        ni_min = ni_min < 0 ? 0 : ni_min;
        if (TV == 2) ni_min = 0;
        auto mfma8 = [&](const double (&af)[MI], const double (&bf)[NI], int nlo) {
#pragma unroll
            for (int ni = nlo; ni < nlo + NI / 2; ++ni) {
                if (FULL || ni >= ni_min) {
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        acc[mi][ni] = GRAM ? mfma_f64_16x16x4(bf[ni], af[mi], acc[mi][ni]) : mfma_f64_16x16x4(af[mi], bf[ni], acc[mi][ni]);
                }
            }
        };
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a0, b0, 0);
        if (TV != 7) lds_frag(a1, b1, cur, 4);
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a0, b0, NI / 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a1, b1, 0);
        lds_frag(a0, b0, cur, 8);
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a1, b1, NI / 2);
        __builtin_amdgcn_sched_barrier(0);
        if (TV != 1 && TV != 3) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // own share of tile t+1 has landed
            __builtin_amdgcn_s_barrier();
        }
        // tile t+2 goes into the stage tile t-1 occupied (free since this barrier).  Issuing the six DMAs keeps a
        // wave from feeding the matrix pipe for a while and the two waves of a SIMD leave the
        // barrier together: column group 0 issues here, column group 1 at the end of the tile.
        //
        // What a full k tile costs beyond its 8,192 cycles of MFMA issue, split with the timing variants (MI355X, N = 4096,
        // 2^21 candidates, launches of eight column groups; stamped builds, cycles per tile | launch time, un-stamped):
        //                                      global_load_lds pieces     buffer_load ... lds pieces (today)
        //   product loop                       8,752 | 30.66 ms           8,536 | 29.94 ms
        //   no barrier (3)                     8,616 | 30.36              8,488 | 30.09
        //   no DMA (4)                         8,456 | 29.69              8,456 | 29.60
        //   no barrier, no DMA (1)             8,440 | 29.64              8,456 | 29.57
        // With global_load_lds the DMA issue was the larger share (296 cycles against 136 for the barrier): every piece took a
        // v_lshl_add_u64 for its 64-bit address, all six into ONE register pair (each had to wait until the load in front of
        // it had read that pair), on the vector issue port that the SIMD partner's MFMAs need.  As buffer loads the pieces
        // take scalar instructions only (glds16): -216 cycles per tile, 506.8 -> 494.2 ms per step on one box, same bits.
        // The rest is 80 cycles of DMA issue, a barrier that now costs nothing (the loop is no faster without it) and 264
        // cycles that remain with neither (the fragment reads and their address arithmetic).
        // Those were split next (variants 5 and 7, which take the run-time loop; one box, two runs each): product 8,528 cycles |
        // 29.80-29.86 ms; every fragment address a loop invariant (5; 2 adds per wave and tile instead of 12) 8,472 | 29.24-29.26;
        // half of the reads as well (7) 8,388 | 30.02-30.03.  Cycles and launch time do not move together here: the launch
        // time is the yardstick.
        // Tried beside it on the same box, all slower, per step: the six pieces spread over the MFMA groups of the half tile,
        // one or two per group (global form 517 / 520 ms against 507; buffer form 508 / 501 against 494: a piece issued among
        // MFMAs stalls more often than six in a row do); s_setprio 1 for waves 4-7 in front of the loop (517 against 507 with the
        // global form, 493.8 against 494.2 = nothing with the buffer form; with the spread pieces 511 / 501); waves 4-7
        // meeting the barrier at the head of their tile, i.e. running half a tile behind waves 0-3 (523 / 519 ms).
        const bool do_stage = pj < nJ && TV != 1 && TV != 4;
        if (do_stage && wq == 0) stage_next();
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a0, b0, 0);
        if (TV != 7) lds_frag(a1, b1, cur, 12);
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a0, b0, NI / 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a1, b1, 0);
        lds_frag(a0, b0, nxt, 0);  // first step of the next tile (stale but in-bounds after the last tile)
        __builtin_amdgcn_sched_barrier(0);
        mfma8(a1, b1, NI / 2);
        __builtin_amdgcn_sched_barrier(0);
        if (do_stage && wq != 0) stage_next();
        if (RING < 0) ring = nxt;
    };
    for (int rr = 0, jb = jb_of(0); jb < nJ; jb = jb_of(++rr)) {
        const int heavy = jb * (BN / BK);
        constexpr std::integral_constant<int, -1> any_stage{};
        int kt = 0;
        if (GPBO_SIGMA_STATIC_RING && TV != 5 && TV != 7) {
            // The full tiles run three at a time from ring position 0: the stage of each is then a compile-time constant
            // and the 12 vector adds per wave and tile that re-base the ds_read2_b64 pairs on the run-time stage fall to 6
            // (same reads, same order, same bits).  Up to two tiles in front (until the ring is at 0) and up to two behind
            // go through the run-time form, as the diagonal block does.  Three separate loops: one loop that branches
            // between the two forms makes hipcc spill 430 registers.  DESIGN 8a has the forms with NO add in the loop
            // (fragment bases kept in registers; compiler-scheduled or inline-assembly reads): all slower than this one.
            for (; ring != 0 && kt < heavy; ++kt) tile_body(std::true_type{}, any_stage, jb, kt);
            for (; kt + 3 <= heavy; kt += 3) {
                tile_body(std::true_type{}, std::integral_constant<int, 0>{}, jb, kt);
                tile_body(std::true_type{}, std::integral_constant<int, 1>{}, jb, kt + 1);
                tile_body(std::true_type{}, std::integral_constant<int, 2>{}, jb, kt + 2);
            }
        }
        for (; kt < heavy; ++kt) tile_body(std::true_type{}, any_stage, jb, kt);
        for (int kt = heavy; kt < heavy + BN / BK; ++kt) tile_body(std::false_type{}, any_stage, jb, kt);
        // column block finished: fold |V|^2 into the row sums (GRAM: V V^T of each tile's 16 candidates into the Gram blocks)
        if (GRAM) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) gram[mi] = mfma_f64_16x16x4(acc[mi][ni][r], acc[mi][ni][r], gram[mi]);
                    acc[mi][ni] = d4_t{0.0, 0.0, 0.0, 0.0};
                }
            continue;
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
#pragma unroll
                for (int r = 0; r < 4; ++r) ss[mi][r] = fma(acc[mi][ni][r], acc[mi][ni][r], ss[mi][r]);
                acc[mi][ni] = d4_t{0.0, 0.0, 0.0, 0.0};
            }
    }
    if (GRAM) {
        // this wave's partial Gram of its 64 candidates over its columns: register r of lane l of tile mi is
        // G[(l >> 4) + 4r][l & 15]; the two diagonal 8 x 8 blocks are the batches 2 t and 2 t + 1 of 16-candidate tile t
        const int p = sp * WQ + wq;
        const int64_t nb8 = ldk / 8;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int64_t t16 = (cand0 + wr * (BM / WR) + mi * 16) / 16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = l4 + 4 * r;
                const bool lo = (r < 2) && (l15 < 8), hi = (r >= 2) && (l15 >= 8);
                if (lo) vbuf[((int64_t)p * nb8 + 2 * t16) * 64 + i * 8 + l15] = gram[mi][r];
                if (hi) vbuf[((int64_t)p * nb8 + 2 * t16 + 1) * 64 + (i - 8) * 8 + (l15 - 8)] = gram[mi][r];
            }
        }
    }

    // ---- row sums: across the 16 lanes that share a candidate row, then across the two column halves
    __syncthreads();
    double *red = smem;  // [WQ][BM]
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = ss[mi][r];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 8);
            if (l15 == 0) red[wq * BM + wr * (BM / WR) + mi * 16 + l4 + 4 * r] = v;
        }
    __syncthreads();

    // (all LDS lives in the one smem[] array: a second __shared__ object makes hipcc wait vmcnt(0) for the
    //  LDS-DMA in front of every k tile's first ds_read)
    double *s_val = smem + WQ * BM;
    int64_t *s_idx = reinterpret_cast<int64_t *>(smem + WQ * BM + 4);
    if (ss_part) {  // (kernel-argument uniform) column-split launch: partial sums only
        if (tid < BM) {
            double ssq = red[tid];
#pragma unroll
            for (int q = 1; q < WQ; ++q) ssq += red[q * BM + tid];
            ss_part[(int64_t)sp * ldk + cand0 + tid] = ssq;
        }
        return;
    }
    if (tid < BM) {
        const int64_t c = cand0 + tid;  // chunk-local candidate
        const bool valid = c < Mc;
        double ssq = red[tid];
#pragma unroll
        for (int q = 1; q < WQ; ++q) ssq += red[q * BM + tid];
        double bv;
        int64_t bi;
        gpbo_candidate_epilogue(ssq, mu_part, nsl, ldk, c, valid, prior_var, ncb > 0 ? GPBO_BOUND_VAR_PAD : 0.0, acq_kind, p0, p1,
                                idx_base, mu_out, sigma_out, acq_out, nullptr, lane, nan_count, bv, bi);
        gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    }
    __syncthreads();
    if (tid == 0) {
        double bv;
        int64_t bi;
        gpbo_argmax_fold(s_val, s_idx, BM / 64, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

// Final reduction over the per-workgroup partials of all chunks: one workgroup.
__global__ __launch_bounds__(256) void argmax_finish_kernel(const double *__restrict__ part_val,
                                                            const int64_t *__restrict__ part_idx, int64_t nparts,
                                                            const unsigned long long *__restrict__ nan_count,
                                                            gpbo_result *__restrict__ result) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63;
    double bv = gpbo_none::val;
    int64_t bi = gpbo_none::idx;
    for (int64_t p = tid; p < nparts; p += 256)
        if (gpbo_better(part_val[p], part_idx[p], bv, bi)) { bv = part_val[p]; bi = part_idx[p]; }
    gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    __syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        result->best_val = bv;
        result->best_idx = bi;
        result->nan_count = (int64_t)*nan_count;
        result->reserved = 0;
    }
}

// Epilogue of a column-split variance launch: |v|^2 = sum of the S partials in index order, then the epilogue
// sigma_acq_kernel calls too (mean from the per-slice partials, sigma, acquisition, dense stores, block arg-max).
__global__ __launch_bounds__(256) void split_finish_kernel(const double *__restrict__ ss_part, int S, int64_t ldk,
                                                           const double *__restrict__ mu_part, int nsl, int64_t Mc,
                                                           double prior_var, int acq_kind, double p0, double p1,
                                                           int64_t idx_base, double *__restrict__ mu_out,
                                                           double *__restrict__ sigma_out, double *__restrict__ acq_out,
                                                           double *__restrict__ var_out,
                                                           double *__restrict__ part_val, int64_t *__restrict__ part_idx,
                                                           unsigned long long *__restrict__ nan_count,
                                                           double var_pad /* > 0: prefix bound, see sigma_acq_kernel */) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t c = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = c < Mc;
    double ssq = 0.0, bv;
    int64_t bi;
    for (int q = 0; q < S; ++q) ssq += ss_part[(int64_t)q * ldk + c];
    gpbo_candidate_epilogue(ssq, mu_part, nsl, ldk, c, valid, prior_var, var_pad, acq_kind, p0, p1, idx_base, mu_out, sigma_out,
                            acq_out, var_out, lane, nan_count, bv, bi);
    gpbo_argmax_post(bv, bi, lane, tid >> 6, s_val, s_idx);
    __syncthreads();
    if (tid == 0) {
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

// Helper stream + events for the K(X*,X) / variance overlap, one set per device, created on first use and kept for the life of
// the process (nothing is retained about the caller's buffers).  ONE scoring call per device at a time records these events: a
// call holds `busy` from its first record to its last (HelperLease), and a caller that finds it taken - another thread on
// another stream - runs the in-order path, which gives the same bits.  The table itself is created under a lock.
struct Helper {
    hipStream_t stream;
    hipEvent_t fork, kdone[2], sdone[2];
    std::mutex busy;
};

Helper *helper_for_current_device() {
    static Helper *tab[64] = {nullptr};
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!tab[dev]) {
        Helper *h = new Helper;
        // (default priority: with the lowest one of hipDeviceGetStreamPriorityRange the unbounded grid stays zero-sum and the
        //  bounded grid gains nothing)
        bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i) {
            ok = ok && hipEventCreateWithFlags(&h->kdone[i], hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&h->sdone[i], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) { delete h; return nullptr; }
        tab[dev] = h;
    }
    return tab[dev];
}

// the helper of this device for the length of a scoring call, or nothing (get() == nullptr) when another call holds it
class HelperLease {
    Helper *h_ = nullptr;

public:
    explicit HelperLease(bool wanted) {
        if (!wanted) return;
        Helper *h = helper_for_current_device();
        if (h && h->busy.try_lock()) h_ = h;
    }
    ~HelperLease() { if (h_) h_->busy.unlock(); }
    HelperLease(const HelperLease &) = delete;
    HelperLease &operator=(const HelperLease &) = delete;
    Helper *get() const { return h_; }
};

static_assert(BN == GPBO_NPAD, "f64_column_groups (host_driver.h) counts column blocks of GPBO_NPAD");

// The workspace of the fp64 pass.  Two chunk buffers when there is more than one chunk (K(X*,X) of chunk c+1 can be built on a
// helper stream while the variance kernel of chunk c runs); with one chunk kst[1] / mup[1] alias the only buffer.
struct PosteriorLayout {
    double *kst[2], *mup[2], *xsc;
    void *prep;   // prefix-bound route (kstar_mfma.hip)
    double *pval;
    int64_t *pidx;
    unsigned long long *nan;
    double *ssp;
    int64_t total, nparts_cap;
    PosteriorLayout(void *work, int64_t Np, int64_t chunk, int64_t M, int split_max = 1) {
        Carver c(work);
        const int64_t nchunks = (M + chunk - 1) / chunk;
        nparts_cap = nchunks * (chunk / BM);
        for (int b = 0; b < (nchunks > 1 ? 2 : 1); ++b) {
            kst[b] = c.take<double>(Np * chunk);
            mup[b] = c.take<double>((Np / GPBO_KS_SLICE) * chunk);
        }
        if (nchunks == 1) { kst[1] = kst[0]; mup[1] = mup[0]; }
        xsc = c.take<double>(Np * GPBO_MAX_D);
        prep = c.take_bytes(gpbo_kstar_mfma_prep_bytes(Np));
        pval = c.take<double>(nparts_cap);
        pidx = c.take<int64_t>(nparts_cap);
        nan = c.take<unsigned long long>(32);   // 256 bytes
        ssp = c.take<double>((split_max > 16 ? split_max : 16) * chunk);
        total = c.total();
    }
};

// number of column-split workgroups per candidate tile for a launch of nblk tiles (1 = the plain kernel)
int split_factor(int64_t nblk, int64_t nJ, int split_max) {
    if (split_max <= 1 || nblk >= 128) return 1;
    int64_t S = (384 + nblk - 1) / nblk;
    if (S > nJ) S = nJ;
    if (S > split_max) S = split_max;
    return S < 1 ? 1 : (int)S;
}

// ================================================================================================
// q-point Monte-Carlo Expected Improvement (BASELINE config 5; not in the reference).
// Candidates are grouped consecutively in batches of q = 8.  For a batch b
//     mu_b  = K*_b alpha,      Sigma_b = K_bb - V_b V_b^T,   V_b = rows of V = K* U belonging to the batch,
//     K_bb  = k(x_i, x_j) with the reference's prior diagonal (1 + 1e-4) + 1e-6,
//     qEI_b = 1/S sum_s max(0, max_j (f_best - xi - (mu_b + chol(Sigma_b) z_s)_j)),   z_s fixed base samples.
// V comes from the variance kernel (vbuf); one wave per batch: Gram of 8 rows of V (coalesced row reads),
// wave reduction, 8x8 Cholesky in registers, S samples spread over the lanes, fixed-order reductions.
// ================================================================================================
constexpr int QQ = 8, QT = QQ * (QQ + 1) / 2;  // 36 lower-triangle entries, index i*(i+1)/2 + j, j <= i

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void qei_kernel(const double *__restrict__ G, int P, int64_t nb8, const double *__restrict__ mu,
                                                  const double *__restrict__ Xs, int d, CovIl2 ls, int64_t nbatch,
                                                  double prior_var, double f_best, double xi,
                                                  const double *__restrict__ Z, int S, int64_t batch_base,
                                                  double *__restrict__ qei_out, double *__restrict__ part_val,
                                                  int64_t *__restrict__ part_idx,
                                                  unsigned long long *__restrict__ nan_count) {
    __shared__ double s_val[4];
    __shared__ int64_t s_idx[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wid;
    const bool valid = b < nbatch;
    const int64_t bb = valid ? b : 0;  // idle waves recompute batch 0 (keeps every shuffle full-wave)
    // V_b V_b^T of the batch: the P partial 8 x 8 blocks the variance launch left (one per column group of its waves and
    // workgroups), summed in partial order - lane e holds entry (e >> 3, e & 7) - then every lane gathers the lower triangle
    double gsum = 0.0;
    for (int q = 0; q < P; ++q) gsum += G[((int64_t)q * nb8 + bb) * 64 + lane];
    double g[QT];
#pragma unroll
    for (int i = 0; i < QQ; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) g[i * (i + 1) / 2 + j] = __shfl(gsum, i * 8 + j);

    // prior covariance of the batch, entry (i, j) by lane t = i(i+1)/2 + j, then gathered by every lane
    double kmine = 0.0;
    if (lane < QT) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= lane) ++i;
        const int j = lane - i * (i + 1) / 2;
        if (i == j) {
            kmine = prior_var;
        } else {
            const double *xi_ = Xs + (bb * QQ + i) * d, *xj_ = Xs + (bb * QQ + j) * d;
            double accd = 0.0;   // cov_r2 over a run-time d, written out
            for (int k = 0; k < d; ++k) {
                const double diff = xi_[k] - xj_[k];
                accd = fma(diff * diff, ls.il2[k], accd);
            }
            kmine = cov_from_r2<GPBO_KERNEL_SE>(accd);
        }
    }
    double L[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) L[t] = __shfl(kmine, t) - g[t];  // Sigma_b, lower triangle

    // in-register Cholesky (every lane redundantly; no divergence)
    bool bad = false;
#pragma unroll
    for (int c = 0; c < QQ; ++c) {
        const double piv = L[c * (c + 1) / 2 + c];
        if (!(piv > 0.0)) bad = true;
        const double dd = sqrt(piv), inv = 1.0 / dd;
        L[c * (c + 1) / 2 + c] = dd;
#pragma unroll
        for (int r = c + 1; r < QQ; ++r) L[r * (r + 1) / 2 + c] *= inv;
#pragma unroll
        for (int r = c + 1; r < QQ; ++r)
#pragma unroll
            for (int q2 = c + 1; q2 <= r; ++q2)
                L[r * (r + 1) / 2 + q2] = fma(-L[r * (r + 1) / 2 + c], L[q2 * (q2 + 1) / 2 + c], L[r * (r + 1) / 2 + q2]);
    }
    double m[QQ];
#pragma unroll
    for (int j = 0; j < QQ; ++j) m[j] = f_best - xi - mu[bb * QQ + j];

    double accs = 0.0;
    for (int s = lane; s < S; s += 64) {
        const double *z = Z + (int64_t)s * QQ;
        double zz[QQ];
#pragma unroll
        for (int j = 0; j < QQ; ++j) zz[j] = z[j];
        double best = 0.0;
#pragma unroll
        for (int j = 0; j < QQ; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k <= j; ++k) t = fma(L[j * (j + 1) / 2 + k], zz[k], t);
            const double imp = m[j] - t;
            best = (imp > best) ? imp : best;  // NaN never raises `best`; it is caught through `bad`
        }
        accs += best;
    }
    double qei = wave_sum(accs) / (double)S;
    bool nanflag = bad || (qei != qei);
#pragma unroll
    for (int j = 0; j < QQ; ++j) nanflag = nanflag || (m[j] != m[j]);
    if (nanflag) qei = __builtin_nan("");
    if (lane == 0) {
        if (valid && qei_out) qei_out[b] = qei;
        if (valid && nanflag) atomicAdd(nan_count, 1ULL);
        s_val[wid] = (valid && !nanflag) ? qei : gpbo_none::val;   // one batch per wave: its record needs no butterfly
        s_idx[wid] = (valid && !nanflag) ? batch_base + b : gpbo_none::idx;
    }
    __syncthreads();
    if (tid == 0) {
        double bv;
        int64_t bi;
        gpbo_argmax_fold(s_val, s_idx, 4, bv, bi);
        part_val[blockIdx.x] = bv;
        part_idx[blockIdx.x] = bi;
    }
}

struct QeiLayout {
    double *kst, *mup, *xsc, *v, *mu, *spv;
    int64_t *spi;
    double *pval;
    int64_t *pidx;
    unsigned long long *nan;
    double *ssp;
    int64_t total;
    QeiLayout(void *work, int64_t Np, int64_t chunk, int64_t M) {
        Carver c(work);
        const int64_t nchunks = (M + chunk - 1) / chunk;
        kst = c.take<double>(Np * chunk);
        mup = c.take<double>((Np / GPBO_KS_SLICE) * chunk);
        xsc = c.take<double>(Np * GPBO_MAX_D);
        v = c.take<double>(64 * (chunk / 8) * 16 * WQ);   // Gram blocks: <= 16 x WQ partials
        mu = c.take<double>(chunk);
        spv = c.take<double>(chunk / BM);
        spi = c.take<int64_t>(chunk / BM);
        const int64_t nparts = nchunks * ((chunk / QQ + 3) / 4);
        pval = c.take<double>(nparts);
        pidx = c.take<int64_t>(nparts);
        nan = c.take<unsigned long long>(32);   // 256 bytes: the reported count and the single-point pass's scratch count
        ssp = c.take<double>(16 * chunk);       // column-group partials (large calls)
        total = c.total();
    }
};

// One variance launch of the acquisition driver: the kernel's arguments once, whichever variant is launched.
struct SigmaLaunch {
    dim3 grid;
    const double *KsT;
    int64_t ldk;
    const double *U;
    int Np;
    const double *mu_part;
    int nsl;
    int64_t Mc;
    double prior_var;
    Acquisition acq;
    int64_t idx_base;
    DenseOut out;       // all null where split_finish_kernel writes the dense outputs
    double *part_val;
    int64_t *part_idx;
    unsigned long long *nan_count;
    double *stamps;     // diagnostics build: where a stamped variant may leave its stamps, or null
    double *ss_part;
    int xg, ntile, ncb;
};

template <int V>
void launch_sigma(const SigmaLaunch &a, hipStream_t st) {
    // (stamped variants: 6 everywhere, 8 and above in the grouped launch only)
    double *stamps = (V == 6 || (a.xg > 1 && V >= 8)) ? a.stamps : nullptr;
    hipLaunchKernelGGL(sigma_acq_kernel<V>, a.grid, dim3(NW * 64), 0, st, a.KsT, a.ldk, a.U, a.Np, a.mu_part, a.nsl, a.Mc,
                       a.prior_var, (int)a.acq.kind, a.acq.p0, a.acq.p1, a.idx_base, a.out.mu, a.out.sigma, a.out.acq,
                       a.part_val, a.part_idx, a.nan_count, stamps, a.ss_part, a.xg, a.ntile, a.ncb);
}

// Timing-only variants of the variance kernel (wrong results; tools/tile_stamps.py uses 6) exist only in a
// diagnostics build (GPBO_DIAG=1 build.sh): the shipped library has no switch into them.
void launch_sigma_variant(const SigmaLaunch &a, hipStream_t st) {
#ifdef GPBO_DIAGNOSTICS
    static const int variant = env_int("GPBO_SIGMA_VARIANT", 0);
    // the grouped launch has variants 1 3 4 5 6 7 9 11 12 13 15, the plain one 1 2 3 4 6; anything else is the product kernel
    const bool have = (a.xg > 1) ? variant != 2 : (variant < 9 && variant != 5 && variant != 7);
    switch (have ? variant : 0) {
        case 1: return launch_sigma<1>(a, st);
        case 3: return launch_sigma<3>(a, st);
        case 4: return launch_sigma<4>(a, st);
        case 6: return launch_sigma<6>(a, st);
        case 9: return launch_sigma<9>(a, st);
        case 11: return launch_sigma<11>(a, st);
        case 12: return launch_sigma<12>(a, st);
        case 5: return launch_sigma<5>(a, st);
        case 7: return launch_sigma<7>(a, st);
        case 13: return launch_sigma<13>(a, st);
        case 15: return launch_sigma<15>(a, st);
        default: return launch_sigma<0>(a, st);
        case 2: return launch_sigma<2>(a, st);
    }
#else
    launch_sigma<0>(a, st);
#endif
}

}  // namespace

int gpbo_launch_split_finish(const double *ss_part, int S, int64_t ldk, const double *mu_part, int nsl, int64_t Mc,
                             double prior_var, const Acquisition &acq, int64_t idx_base, const DenseOut &out,
                             double *part_val, int64_t *part_idx, unsigned long long *nan_count, hipStream_t st) {
    const int64_t nb = (Mc + 255) / 256;
    hipLaunchKernelGGL(split_finish_kernel, dim3((unsigned)nb), dim3(256), 0, st, ss_part, S, ldk, mu_part, nsl, Mc, prior_var,
                       (int)acq.kind, acq.p0, acq.p1, idx_base, out.mu, out.sigma, out.acq, out.var, part_val, part_idx,
                       nan_count, 0.0);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

int gpbo_launch_argmax_finish(const double *part_val, const int64_t *part_idx, int64_t nparts,
                              const unsigned long long *nan_count, gpbo_result *result, hipStream_t st) {
    hipLaunchKernelGGL(argmax_finish_kernel, dim3(1), dim3(256), 0, st, part_val, part_idx, nparts, nan_count, result);
    GPBO_CHECK_LAUNCH();
    return GPBO_OK;
}

extern "C" int64_t gpbo_posterior_workspace_bytes(int64_t Np, int64_t chunk, int64_t M) {
    return gpbo_posterior_workspace_bytes_split(Np, chunk, M, 1);
}

extern "C" int gpbo_posterior_acq_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                      const double *ls_host, const double *U, const double *alpha, double prior_var,
                                      int32_t acq_kind, double p0, double p1, double diag_add, int64_t idx_offset,
                                      int64_t chunk, double *mu_out, double *sigma_out, double *acq_out,
                                      gpbo_result *result, void *work, int64_t work_bytes, gpbo_profile *prof,
                                      void *stream) {
    return gpbo_posterior_acq_kern_f64(Xs, M, X, N, Np, d, ls_host, GPBO_KERNEL_SE, U, alpha, prior_var, acq_kind, p0, p1, diag_add,
                                       idx_offset, chunk, mu_out, sigma_out, acq_out, result, work, work_bytes, prof, stream);
}

// (the covariance family reaches the K(X*,X) launches only: the variance kernel, the epilogues and the arg-max work on K*^T)
extern "C" int gpbo_posterior_acq_kern_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                           const double *ls_host, int32_t kernel, const double *U, const double *alpha,
                                           double prior_var, int32_t acq_kind, double p0, double p1, double diag_add,
                                           int64_t idx_offset, int64_t chunk, double *mu_out, double *sigma_out,
                                           double *acq_out, gpbo_result *result, void *work, int64_t work_bytes,
                                           gpbo_profile *prof, void *stream) {
    return gpbo_posterior_acq_f64_split(Xs, M, {X, N, Np, d, ls_host, U, alpha, prior_var, kernel}, {acq_kind, p0, p1}, diag_add,
                                        idx_offset, chunk, {mu_out, sigma_out, acq_out, nullptr}, result, work, work_bytes,
                                        prof, 1, 0, stream);
}

// The prefix-bound screen's first pass (rescore.hip, gpbo_bound_select_f64): the mean over all N observations, the
// variance product over the FIRST n_prefix columns of V only.  |v_c|^2 summed over a prefix of its components is a lower
// bound of the whole sum, so sigma_out / acq_out hold UPPER bounds of the fp64 path's values (both acquisitions increase
// with sigma; LCB only for explore >= 0).  K*^T is stored for the first n_prefix observations only.
extern "C" int gpbo_posterior_prefix_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                         const double *ls_host, const double *U, const double *alpha, double prior_var,
                                         int32_t acq_kind, double p0, double p1, int64_t idx_offset, int64_t chunk,
                                         int64_t n_prefix, double *mu_out, double *sigma_ub_out, double *acq_ub_out,
                                         gpbo_result *result, void *work, int64_t work_bytes, gpbo_profile *prof,
                                         void *stream) {
    if (n_prefix < BN || n_prefix % BN || n_prefix > Np) return GPBO_ERR_ARG;
    if (acq_kind == GPBO_ACQ_LCB && !(p0 >= 0.0)) return GPBO_ERR_ARG;
    return gpbo_posterior_acq_f64_split(Xs, M, {X, N, Np, d, ls_host, U, alpha, prior_var}, {acq_kind, p0, p1}, 0.0,
                                        idx_offset, chunk, {mu_out, sigma_ub_out, acq_ub_out, nullptr}, result, work,
                                        work_bytes, prof, 1, n_prefix, stream);
}

int64_t gpbo_posterior_workspace_bytes_split(int64_t Np, int64_t chunk, int64_t M, int split_max) {
    if (!np_ok(Np) || !chunk_ok(chunk) || M < 1) return GPBO_ERR_ARG;
    return PosteriorLayout(nullptr, Np, chunk, M, split_max).total;
}

const double *gpbo_posterior_chunk_image(const void *work, int64_t Np, int64_t chunk, int64_t M) {
    return PosteriorLayout(const_cast<void *>(work), Np, chunk, M).kst[0];
}

// split_max > 1: launches of fewer than 128 candidate tiles are split over the column blocks of V (the re-scoring
// of a few survivors: one workgroup per 256 candidates would take N^2/2 MFMA-bound k tiles on ONE compute unit).
// The partial sums are combined in a fixed order, so results are deterministic; they differ from the unsplit
// kernel's by the rounding of a different summation order (~1e-16 relative).
int gpbo_posterior_acq_f64_split(const double *Xs, int64_t M, const GpModel &gp, const Acquisition &acq, double diag_add,
                                 int64_t idx_offset, int64_t chunk, const DenseOut &out, gpbo_result *result, void *work,
                                 int64_t work_bytes, gpbo_profile *prof, int split_max,
                                 int64_t n_prefix /* 0: everything; else see gpbo_posterior_prefix_f64 */, void *stream) {
    const double *X = gp.X, *U = gp.U, *alpha = gp.alpha, *ls_host = gp.ls_host;
    const int64_t N = gp.N, Np = gp.Np;
    const int32_t d = gp.d;
    if (!Xs || !X || !U || !alpha || !result || !work) return GPBO_ERR_ARG;
    // (a Matern family: never with the prefix bound, whose mean comes from the squared-exponential kstar_mfma.hip)
    if (!kernel_ok(gp.kernel, d, diag_add) || (gp.kernel != GPBO_KERNEL_SE && n_prefix != 0)) return GPBO_ERR_ARG;
    if (n_prefix < 0 || n_prefix > Np || n_prefix % BN || (n_prefix && diag_add != 0.0)) return GPBO_ERR_ARG;
    if (M < 1 || N < 1 || Np != gpbo_padded_n(N) || Np > (1 << 20)) return GPBO_ERR_ARG;
    if (!chunk_ok(chunk)) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq.kind)) return GPBO_ERR_ARG;
    if (!aligned_to(work, 256) || !aligned_to(U, 16)) return GPBO_ERR_ARG;
    const PosteriorLayout L(work, Np, chunk, M, split_max);
    if (work_bytes < L.total) return GPBO_ERR_WORKSPACE;
    hipStream_t st = gpbo_stream(stream);
    // prefix-bound route: K(X*,X) with the pair distances on the matrix cores and the mean reported from below by its error
    // bound (kstar_mfma.hip; GPBO_PREFIX_VALU=1: the difference-form kernel instead, for A/B runs)
    static const bool prefix_valu = env_flag("GPBO_PREFIX_VALU");
    static const bool overlap_env = env_flag("GPBO_OVERLAP");
    // (and only while the unused rows of the K*^T slab can take that launch's mean partials)
    const bool kstar_mfma = n_prefix > 0 && !prefix_valu && !overlap_env && n_prefix + n_prefix / GPBO_KS_SLICE <= Np;
    const bool anyd = d > GPBO_MAX_D;   // slow path of the fp64 route: no unrolled registers, no pre-scaled copy
    if (anyd && (n_prefix > 0 || d > GPBO_MAX_D_ANY)) return GPBO_ERR_ARG;
    if (anyd) {
        if (hipMemsetAsync(L.nan, 0, sizeof(unsigned long long), st) != hipSuccess) return GPBO_ERR_LAUNCH;
    } else {
        // observations / (ls sqrt 2), once per call; the same launch clears the NaN counter
        int rc0 = gpbo_scale_points_launch(X, N, Np, d, ls_host, L.xsc, L.nan, stream);
        if (rc0 != GPBO_OK) return rc0;
    }
    if (kstar_mfma) {
        int rc0 = gpbo_kstar_mfma_prep(X, N, Np, d, ls_host, alpha, L.prep, stream);
        if (rc0 != GPBO_OK) return rc0;
    }

    // K(X*,X) of chunk c + 1 beside the variance kernel of chunk c.  As two ordinary launches this is zero-sum:
    // a variance workgroup holds 448 of a SIMD's 512 registers and all but 4 KiB of the LDS, a 72-register K(X*,X) workgroup never
    // shares a compute unit with it, and the two kernels time-slice whole compute units (N = 4096, 2^21 candidates: the variance
    // launches 29.51 -> 30.16 ms, the step 485.8 -> 485.6 ms; the 64-register form in an unbounded grid: 30.29 ms, 487.7 ms).
    // The co-resident form of kstar_mu_kernel (kernel_build.hip) in its bounded grid - one workgroup per compute unit, resident
    // beside the variance workgroups from the start of the launch - costs the variance launch 0.34 ms (29.51 -> 29.85) for a
    // build that takes 0.70 ms alone and issues 0.5 ms of fp64 vector instructions: 480.8 against 485.8 ms per step.  So an fp64
    // vector instruction of another wave does take the SIMD's issue slot from the fp64 MFMA, but only about two thirds of the
    // build's vector issue shows up as lost matrix time, and none of its store time.
    // Default where that form exists, the call has more than one chunk and takes the grouped launch (below that the launches
    // are too short to matter); GPBO_OVERLAP=0 switches it off (the A/B switch), any other value switches it on for every call
    // of more than one chunk (the co-resident form where it exists, the stand-alone form elsewhere).
    const int64_t nchunks = (M + chunk - 1) / chunk;
    static const int overlap_mode = env_int("GPBO_OVERLAP", -1);   // -1: not set
    const bool beside = !anyd && !kstar_mfma && gpbo_kstar_beside_ok(d, gp.kernel, diag_add, chunk);
    const bool overlap = nchunks > 1 && (overlap_env || (overlap_mode < 0 && beside && split_max == 1 && n_prefix == 0 &&
                                                         f64_column_groups(M, Np) > 1));
    // (a second caller on this device while this call records: in order, the same bits)
    const HelperLease lease(overlap);
    Helper *hp = lease.get();
    // Fork: the helper stream builds K(X*,X)+mu of chunk c+1 (fp64 VALU + HBM writes) while the caller's stream runs the
    // variance kernel of chunk c (matrix cores); two chunk buffers, events both ways.  Chunk 0 has nothing to run beside: it is
    // built on the caller's stream in the stand-alone form, and the fork follows it.
    hipStream_t ks = hp ? hp->stream : st;
    // partials of the mean per candidate: 64-observation slices, coarser ones from the matrix-core K(X*,X) kernel
    const int nsl = kstar_mfma ? (int)(Np / gpbo_kstar_mfma_slice(Np)) : (int)(Np / GPBO_KS_SLICE);
    ProfileRecorder slots(prof);
    auto launch_kstar = [&](int64_t c) -> int {
        const int64_t s = c * chunk;
        const int64_t Mc = (M - s < chunk) ? (M - s) : chunk;
        const int b = (int)(c & 1);
        hipStream_t kst = (hp && c > 0) ? ks : st;
        // The K(X*,X) interval of a slot is timed where the launch runs alone on the caller's stream: every chunk in the in-order
        // mode, chunk 0 of a call in the overlapped mode - so the figure read from the slots stays the stand-alone build's; the
        // builds that run beside a variance launch show up in that launch's interval (begin / end below), which is what they cost.
        // (a build on the helper stream is enqueued while the slot of the chunk before it is still open: marked untimed below)
        if ((!hp || c == 0) && !slots.kstar(st, c > 0)) return GPBO_ERR_LAUNCH;
        int rc;
        if (kstar_mfma) {
            // The MEAN of all N observations from the matrix-core kernel (expanded distances; reported from below by its
            // own error bound), but the n_prefix stored rows of K*^T from the difference-form kernel of the plain pass:
            // the expanded form's entry error grows with the points' distance from the centroid in length-scale units
            // (unnormalised inputs), is amplified by |U| and would need a data-dependent variance pad; with the plain
            // pass's own entries |v[:J]|^2 is a partial sum of the very squares the plain pass adds up, so the bound
            // holds for any inputs.  Costs n_prefix / N of the fp64-VALU kernel: 6 % at N / 16.
            rc = gpbo_kstar_mu_mfma(Xs + s * d, Mc, N, Np, d, ls_host, alpha, L.prep, L.kst[b], chunk, L.mup[b], 0, kst);
            if (rc != GPBO_OK) return rc;
            const int64_t nrow = (N < n_prefix) ? N : n_prefix;
            // (its mean partials - of the first n_prefix observations only - are not wanted: they go to rows of the K*^T
            //  slab that the prefix mode neither writes nor reads, [n_prefix, n_prefix + n_prefix / 64))
            rc = gpbo_kstar_mu_rows(Xs + s * d, Mc, L.xsc, nrow, n_prefix, d, ls_host, GPBO_KERNEL_SE, alpha, 0.0, idx_offset + s,
                                    L.kst[b], chunk, L.kst[b] + n_prefix * chunk, n_prefix, 0, kst);
        } else if (anyd) {
            rc = gpbo_kstar_mu_anyd(Xs + s * d, Mc, X, N, Np, d, ls_host, alpha, diag_add, idx_offset + s, L.kst[b], chunk,
                                    L.mup[b], kst);
        } else {
            rc = gpbo_kstar_mu_rows(Xs + s * d, Mc, L.xsc, N, Np, d, ls_host, gp.kernel, alpha, diag_add, idx_offset + s, L.kst[b],
                                    chunk, L.mup[b], n_prefix ? n_prefix : Np, hp && c > 0 && beside, kst);
        }
        if (rc != GPBO_OK) return rc;
        if (hp && c > 0 && hipEventRecord(hp->kdone[b], ks) != hipSuccess) return GPBO_ERR_LAUNCH;
        return GPBO_OK;
    };
    int rc = launch_kstar(0);
    if (rc != GPBO_OK) return rc;
    if (hp) {
        if (hipEventRecord(hp->fork, st) != hipSuccess || hipStreamWaitEvent(ks, hp->fork, 0) != hipSuccess)
            return GPBO_ERR_LAUNCH;
    }
    int64_t nparts = 0;
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t s = c * chunk;
        const int64_t Mc = (M - s < chunk) ? (M - s) : chunk;
        const int b = (int)(c & 1);
        if (hp && c + 1 < nchunks) {
            // buffer (c+1)&1 was last read by the variance kernel of chunk c-1
            if (c >= 1 && hipStreamWaitEvent(ks, hp->sdone[(c + 1) & 1], 0) != hipSuccess) return GPBO_ERR_LAUNCH;
            rc = launch_kstar(c + 1);
            if (rc != GPBO_OK) return rc;
        }
        if (hp && c > 0 && hipStreamWaitEvent(st, hp->kdone[b], 0) != hipSuccess) return GPBO_ERR_LAUNCH;
        const int64_t nblk = (Mc + BM - 1) / BM;
        if (hp && c > 0 && !slots.kstar(st, false, false)) return GPBO_ERR_LAUNCH;
        if (!slots.begin(st)) return GPBO_ERR_LAUNCH;
        const int S = split_factor(nblk, (n_prefix ? n_prefix : Np) / BN, split_max);
        // Column groups on one XCD for large calls (see the kernel): measured on MI355X at N = 4096, 2^21 candidates,
        // same box: 543 -> 509 ms per step with 8 groups (16: 512), the variance launches 32.9 -> 30.7 ms.
        const int xg = (S == 1 && n_prefix == 0) ? f64_column_groups(M, Np) : 1;
        const DenseOut o = out.at(s);
        SigmaLaunch a = {dim3((unsigned)nblk), L.kst[b], chunk, U, (int)Np, L.mup[b], nsl, Mc, gp.prior_var, acq,
                         idx_offset + s, o, L.pval + nparts, L.pidx + nparts, L.nan,
                         // (the stamps of a stamped variant go to the other chunk buffer, free during the last chunk)
                         (c == nchunks - 1 && nchunks > 1) ? L.kst[(c + 1) & 1] : nullptr, nullptr, 1, (int)nblk,
                         (int)(n_prefix / BN)};
        if (xg > 1 || S > 1) {   // partial sums to L.ssp, the epilogue in split_finish_kernel
            a.grid = (xg > 1) ? dim3((unsigned)((nblk + 7) / 8 * 8 * xg)) : dim3((unsigned)nblk, (unsigned)S);
            a.out = {nullptr, nullptr, nullptr, nullptr};
            a.ss_part = L.ssp;
            a.xg = xg;
            if (xg > 1) launch_sigma_variant(a, st);
            else launch_sigma<0>(a, st);
            hipLaunchKernelGGL(split_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, st, L.ssp, xg > 1 ? xg : S, chunk,
                               L.mup[b], nsl, Mc, gp.prior_var, (int)acq.kind, acq.p0, acq.p1, idx_offset + s, o.mu, o.sigma,
                               o.acq, (double *)nullptr, L.pval + nparts, L.pidx + nparts, L.nan,
                               n_prefix ? GPBO_BOUND_VAR_PAD : 0.0);
        } else {
            launch_sigma_variant(a, st);
        }
        if (!slots.end(st, Mc)) return GPBO_ERR_LAUNCH;
        GPBO_CHECK_LAUNCH();
        if (hp && hipEventRecord(hp->sdone[b], st) != hipSuccess) return GPBO_ERR_LAUNCH;
        if (!hp && c + 1 < nchunks) {
            rc = launch_kstar(c + 1);
            if (rc != GPBO_OK) return rc;
        }
        nparts += nblk;
    }
    return gpbo_launch_argmax_finish(L.pval, L.pidx, nparts, L.nan, result, st);
}

namespace {
// Acquisition over dense mu / sigma that are already on the device (used when the caller asks for a second acquisition on the
// same posterior, e.g. lower_confidence_bound(explore != 4)): an instance of dense_acq_kernel (dense_acq.h).
struct AcqScore {
    const double *__restrict__ mu, *__restrict__ sigma;
    double *__restrict__ acq_out;
    double p0, p1;
    int32_t kind, pad;
    __device__ __forceinline__ double operator()(int64_t c) const {
        const double a = gpbo_acquisition(kind, mu[c], sigma[c], p0, p1);
        if (acq_out) acq_out[c] = a;
        return a;
    }
};
}  // namespace

extern "C" int64_t gpbo_acq_workspace_bytes(void) { return DenseAcqScratch::bytes(); }

extern "C" int gpbo_acq_argmax_f64(const double *mu, const double *sigma, int64_t M, int32_t acq_kind, double p0,
                                   double p1, int64_t idx_offset, double *acq_out, gpbo_result *result, void *work,
                                   int64_t work_bytes, void *stream) {
    if (!mu || !sigma || !result || !work || M < 1) return GPBO_ERR_ARG;
    if (!acq_kind_ok(acq_kind)) return GPBO_ERR_ARG;
    if (work_bytes < DenseAcqScratch::bytes()) return GPBO_ERR_WORKSPACE;
    const AcqScore sc = {mu, sigma, acq_out, p0, p1, acq_kind, 0};
    return dense_acq_launch(M, sc, idx_offset, DenseAcqScratch(work), result, gpbo_stream(stream));
}

extern "C" int64_t gpbo_qei_workspace_bytes(int64_t Np, int64_t chunk, int64_t M) {
    if (!np_ok(Np) || !chunk_ok(chunk) || M < 1) return GPBO_ERR_ARG;
    return QeiLayout(nullptr, Np, chunk, M).total;
}

extern "C" int gpbo_posterior_qei_f64(const double *Xs, int64_t M, const double *X, int64_t N, int64_t Np, int32_t d,
                                      const double *ls_host, const double *U, const double *alpha, double prior_var,
                                      double f_best, double xi, const double *Z, int32_t S, int64_t batch_offset,
                                      int64_t chunk, double *qei_out, gpbo_result *result, void *work,
                                      int64_t work_bytes, gpbo_profile *prof, void *stream) {
    if (!Xs || !X || !U || !alpha || !Z || !result || !work) return GPBO_ERR_ARG;
    if (M < QQ || M % QQ || N < 1 || Np != gpbo_padded_n(N) || S < 1 || d < 1 || d > GPBO_MAX_D) return GPBO_ERR_ARG;
    if (!chunk_ok(chunk)) return GPBO_ERR_ARG;
    if (!aligned_to(work, 256) || !aligned_to(U, 16)) return GPBO_ERR_ARG;
    const QeiLayout L(work, Np, chunk, M);
    if (work_bytes < L.total) return GPBO_ERR_WORKSPACE;
    CovIl2 ls;
    for (int k = 0; k < GPBO_MAX_D; ++k) ls.il2[k] = 0.0;
    if (!length_scale_scalings(ls_host, d, ls.il2, nullptr)) return GPBO_ERR_ARG;
    hipStream_t st = gpbo_stream(stream);
    unsigned long long *nan_scratch = L.nan + 8;  // NaN count of the single-point pass (not reported)
    if (hipMemsetAsync(L.nan, 0, 256, st) != hipSuccess) return GPBO_ERR_LAUNCH;
    int rc = gpbo_scale_points_f64(X, N, Np, d, ls_host, L.xsc, stream);
    if (rc != GPBO_OK) return rc;
    int64_t nparts = 0;
    ProfileRecorder slots(prof);
    for (int64_t s = 0; s < M; s += chunk) {
        const int64_t Mc = (M - s < chunk) ? (M - s) : chunk;
        // one profile slot per chunk: kbegin | K(X*,X) | begin | variance launch (+ its finish) | end | qEI launch | qend
        // (the qEI launch lies between a slot's end and the next K(X*,X) launch: no chaining)
        if (!slots.kstar(st, false)) return GPBO_ERR_LAUNCH;
        rc = gpbo_kstar_mu_f64(Xs + s * d, Mc, L.xsc, N, Np, d, ls_host, alpha, 0.0, 0, L.kst, chunk, L.mup, stream);
        if (rc != GPBO_OK) return rc;
        if (!slots.begin(st)) return GPBO_ERR_LAUNCH;
        const int64_t nblk = (Mc + BM - 1) / BM;
        // the variance kernel in its GRAM form leaves the batches' partial V V^T blocks (vbuf) and mu; its own single-point
        // acquisition result is ignored.  Large calls: column groups on one XCD as in gpbo_posterior_acq_f64 (each group
        // leaves the Gram partials of its column blocks; the mean then comes from split_finish_kernel).
        const int xg = f64_column_groups(M, Np);
        const int gram_parts = xg * WQ;   // partial Gram blocks per batch: one per column group of waves and of workgroups
        double *ss_part = xg > 1 ? L.ssp : nullptr;
        const int64_t grid = xg > 1 ? (nblk + 7) / 8 * 8 * xg : nblk;
        hipLaunchKernelGGL((sigma_acq_kernel<0, true>), dim3((unsigned)grid), dim3(NW * 64), 0, st, L.kst, chunk, U, (int)Np, L.mup,
                           (int)(Np / GPBO_KS_SLICE), Mc, prior_var, (int)GPBO_ACQ_LCB, 0.0, 0.0, (int64_t)0,
                           xg > 1 ? (double *)nullptr : L.mu, (double *)nullptr, (double *)nullptr, L.spv, L.spi, nan_scratch, L.v,
                           ss_part, xg, (int)nblk, 0);
        if (xg > 1)
            hipLaunchKernelGGL(split_finish_kernel, dim3((unsigned)nblk), dim3(256), 0, st, ss_part, xg, chunk, L.mup,
                               (int)(Np / GPBO_KS_SLICE), Mc, prior_var, (int)GPBO_ACQ_LCB, 0.0, 0.0, (int64_t)0, L.mu,
                               (double *)nullptr, (double *)nullptr, (double *)nullptr, L.spv, L.spi, nan_scratch, 0.0);
        GPBO_CHECK_LAUNCH();
        if (!slots.end_open(st)) return GPBO_ERR_LAUNCH;
        const int64_t nbatch = Mc / QQ;
        const int64_t qblk = (nbatch + 3) / 4;
        hipLaunchKernelGGL(qei_kernel, dim3((unsigned)qblk), dim3(256), 0, st, L.v, gram_parts, chunk / 8, L.mu, Xs + s * d, (int)d, ls, nbatch,
                           prior_var, f_best, xi, Z, (int)S, batch_offset + s / QQ, qei_out ? qei_out + s / QQ : nullptr,
                           L.pval + nparts, L.pidx + nparts, L.nan);
        GPBO_CHECK_LAUNCH();
        if (!slots.qend(st, Mc)) return GPBO_ERR_LAUNCH;
        nparts += qblk;
    }
    return gpbo_launch_argmax_finish(L.pval, L.pidx, nparts, L.nan, result, st);
}
