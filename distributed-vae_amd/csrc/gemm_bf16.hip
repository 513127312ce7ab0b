// The five D x H GEMMs of the train step on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16), in two precisions:
//
//   * mmvae_hyper.gemm_bf16 == 1 -- BASELINE.json configs[2] ("bf16, DP over 8 GPUs"): operands ROUNDED to bf16;
//   * mmvae_hyper.gemm_bf16 == 2 -- "fp32x3", the library's fp32 engine: every fp32 operand split EXACTLY into three bf16
//     slices, six slice products per product (see Eng<NP> below; k_presplit, k_x3_gemm, k_x3_small, k_x3_fc11g; DESIGN.md
//     section 14).  It also serves the small-layer gradient products.
//
// What follows describes the shared tile engine in its one-plane (bf16) form.  Operands are rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) on their way
// into LDS, products accumulate in fp32 on v_mfma_f32_32x32x16_bf16 (2.5 PFLOP/s dense: 16 x the fp32 matrix rate), and
// everything else of the step -- BatchNorm, the softmaxes, KL / coupling terms, the reconstruction-loss epilogue, the
// slab reduction, Adam, the parameters themselves -- stays fp32 (SURVEY.md section 7 "Numerical range").  With the
// matrix pipe 16 x faster these kernels are bound by how fast a CU can pull its tiles out of L2 / HBM, so they share ONE
// simple tile engine instead of five hand-scheduled instruction streams:
//
//   C[m][n] (+ epilogue) = sum_k A(m, k) * B(n, k),  block tile 128 x 128, 256 threads = 2 x 2 waves of 64 x 64
//   (2 x 2 MFMA tiles of 32 x 32), K tile 64 = 4 MFMA steps of 16; one LDS buffer per operand, [row][k] bf16 with k
//   contiguous (row stride 144 B), so a lane's MFMA fragment (8 consecutive k of one row) is one ds_read_b128.
//
// An operand is described by how (row, k) maps to memory:
//   KMAJOR   ptr[row * ld + k]   k contiguous in memory   (x, W1, d10, W11 rows, dZ11 rows)
//   KMINOR   ptr[k * ld + row]   rows contiguous          (the batch-reduced GEMMs: dZ1, x, dZ11, d10 as [b][.];
//                                                          W11 as [j][h] for d(d10)): staged as they lie, [k][row],
//                                                          and transposed by the LDS read (ds_read_b64_tr_b16)
// plus optional decorations: the bit-packed dropout keep-mask of x (k_make_xbits) and a ones column (bias gradient).
// fc11's bias is added in fp32 by the epilogue (it is not a GEMM operand of the reference either).
//
//   fc1 forward      C[cell][h]  = x~[cell][:] . W1[h][:]            A KMAJOR+mask, B KMAJOR     -> split-K slabs
//   fc11 + loss      z[cell][j]  = d10[cell][:] . W11[j][:] (+ b11) A KMAJOR, B KMAJOR          -> dZ11, loss partials
//   d(d10)           g[cell][h]  = dZ11[cell][:] . W11[:][h]         A KMAJOR, B KMINOR          -> gene-split slabs
//   dW1              G[h][d]     = dZ1[:][h] . x~[:][d]              A KMINOR, B KMINOR+mask     -> batch-split slabs
//   [dW11 | db11]    G[j][h]     = dZ11[:][j] . [d10 | 1][:][h]      A KMINOR, B KMINOR+ones col -> batch-split slabs
// The outputs have the layouts of the fp32 kernels (gemm_fast.hip), so k_fc1_epi, the decoder chain and k_reduce are
// shared.  Reference arithmetic: mmidas/nn_model.py:263-287 (fc1, fc11), :542-546 (loss), autograd of both.
#include "common.hpp"

namespace mmvae {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));


constexpr int BT = 128;          // block tile (both ways)
constexpr int KT = 64;           // K tile of the one-plane engine (the fc11 kernels below use it directly)
constexpr int LDB = 36;          // its KMAJOR LDS image [row][k]: row stride in dwords, 64 bf16 = 32 dwords + 4 (16-byte aligned rows)
constexpr int LDK = 136;         // KMINOR LDS image [k][row]: k-row stride in bf16, 128 rows + 8 (8-byte aligned)

// The engine exists in two precisions, selected by the number of bf16 PLANES an operand has in LDS:
//   NP = 1  bf16 operands (BASELINE configs[2]): K tile 64, two K tiles in LDS.
//   NP = 3  fp32 operands, split exactly into three bf16 slices on their way into LDS, x = x1 + x2 + x3 with
//           x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2) (8 + 8 + 8 significand bits; both differences are exact
//           in fp32, and x3 is exact).  The product a b is formed from six of the nine slice products, a1 b1 + (a1 b2 + a2 b1)
//           + (a1 b3 + a2 b2 + a3 b1); each is exact in the fp32 accumulator's input (8 x 8 bits), the dropped ones are
//           <= 2^-26 |a b|, below the fp32 rounding of the accumulation itself.  Six v_mfma_f32_32x32x16_bf16 do the work
//           of eight v_mfma_f32_32x32x2_f32 in 6/64 of their time (the bf16 matrix rate is 16 x the fp32 one), so the
//           fp32 configuration's large GEMMs leave the matrix pipe's roof and become memory-bound like the bf16 ones.
//           K tile 32, one K tile in LDS (3 planes x 2 operands x 10 KB = 60 KB: two workgroups per CU).
template <int NP>
struct Eng {
    static constexpr int KT = NP == 1 ? 64 : 32;
    static constexpr int NQ = KT / 8;            // 16-byte pieces per thread per operand and K tile
    static constexpr int LDB = KT / 2 + 4;       // KMAJOR image row stride in dwords (36 / 20: conflict-free ds_read_b128)
    static constexpr int PLANE = BT * LDB;       // dwords of one plane's image (the KMINOR image, KT x LDK bf16, fits in it)
    // KMINOR image [k][row]: k-row pitch in bf16.  A transposing read (ds_read_b64_tr_b16) takes, per 16 lanes, 4 k rows x
    // 16 row-columns (8 bytes per lane), 32 lanes per LDS cycle: with a pitch of 68 dwords (136 bf16) k rows q and q + 1
    // land 4 banks apart and collide with the neighbouring lanes' 8-byte reads (PMC: SQ_LDS_BANK_CONFLICT = 31 % of the
    // busy cycles of dW1 / dW11); 80 dwords (160 bf16) puts them 16 banks apart -- the four k rows of both 16-lane
    // groups tile the 64 banks exactly -- and 32 x 160 bf16 is exactly one plane.  The one-plane engine (K tile 64)
    // has no room for that pitch and keeps 136.
    static constexpr int LDK = NP == 1 ? 136 : 160;
    static constexpr int NBUF = NP == 1 ? 2 : 1;
};

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    bf16x2 v;
    v[0] = (__bf16)a;
    v[1] = (__bf16)b;
    return __builtin_bit_cast(unsigned, v);
}
// (cvt_pk_bf16 and split3 -- the three bf16 slices of two fp32 values -- live in common.hpp: the chain kernels write
// slice planes too)

struct Operand {
    const float* ptr;        // this arm's matrix
    int64_t ld;              // leading dimension (floats)
    int rows, K;             // rows (m or n) that exist in memory and k extent
    int kminor;              // 0: ptr[row * ld + k]; 1: ptr[k * ld + row]
    const uint32_t* bits;    // optional keep-mask of x: bit (col & 31) of bits[cell * wpr + (col >> 5)], cell / col = (row, k) or (k, row)
    int wpr;
    int ones_row;            // KMINOR: row index that reads as 1.0 for every k < K (bias gradient), or -1
    // fp32x3 engine only: the operand's three bf16 slice planes, prepared once per step by k_presplit for the SMALL operand
    // of each large GEMM (W1, W11, dZ1, [d10 | 1]; every block tile of the GEMM would otherwise split the same values
    // again): [3][R][C] bf16 in the orientation of the fp32 matrix, zero-padded to whole tiles
    const unsigned short* pl;
    int64_t pl_plane, pl_arm;    // elements per plane / per arm
    int pl_ld;                   // row pitch (elements)
    // row indirection (the batch is never materialised: mmvae_train_step_rows): logical row / k index i of the operand lies
    // at ptr[rowmap[i] .. + ld) instead of ptr[i * ld ..); rowmap: uint32 [map_n] element offsets, nrec: floats addressable
    // from ptr (< 2^30).  The keep-mask words stay indexed by the logical index.
    const unsigned* rowmap;
    int64_t nrec;
    int map_n;
    // bf16 storage (the bf16 configuration on a bf16 copy of x / a bf16 dZ11, mmvae_train_step_rows(data_bf16)): ptr addresses
    // 2-byte elements (same ld, in elements); read through oct_load / oct_store below.  rows, K, ld: multiples of 8.
    int src16;
};

// One K tile of an operand in flight: rows [r0, r0 + 128) x k [k0, k0 + KT).  `load` only REQUESTS the data (NQ
// float4 and their mask words per thread; nothing touches the values, so the requests of both operands issue back to
// back and land while the MFMAs of the previous tile run); `store` masks, rounds to bf16 (or splits into the three
// slices) and writes the LDS image(s) ([128][LDB] dwords, bf16 pairs along k, zero outside the operand).
template <bool BITS, int NQ = 8>
struct TileRegsT {
    float4 v[NQ];
    uint32_t wd[BITS ? NQ : 1];   // keep-mask words (only operands that carry a mask hold them)
};

// Loads go through buffer instructions: the operand's base sits in an SGPR descriptor and a piece is addressed by a
// 32-bit per-lane byte offset that is computed ONCE per block tile (PieceCtx) plus a uniform term for what is the same for
// every lane: the K tile and the piece's own step (one addition per request).  No 64-bit pointers stay live across the pipeline (sixteen of them
// per thread cost 32 VGPRs and pushed the kernel into scratch) and nothing is clamped: a piece that does not exist -- a row
// beyond the operand, a k beyond the K range -- asks for the lane offset PIECE_OOB, which lies past every descriptor's
// range, so the load returns 0 and touches no memory.
// Every operand has ld % 4 == 0, K % 4 == 0 and < 4 GB per arm.
constexpr unsigned PIECE_OOB = 0xFFFFFFF0u;
struct OperandDev {
    __amdgpu_buffer_rsrc_t rs, rb;   // matrix, mask words (no mask: a range of 0 bytes)
    __amdgpu_buffer_rsrc_t rm;       // row map (row indirection; see Operand::rowmap)
    const unsigned* mp;              // the same map as a pointer: K-minor operands read it with scalar loads (map_request)
    int ld, rows, K, wpr, ones_row;
    bool bits;
    unsigned nomask;                 // ORed onto a mask word: 0, or all ones for an operand without a mask (whose words read 0)
    float4 bn_sub, bn_mul;           // BN = true (k_x3_small): this thread's four rows read (v - bn_sub) * bn_mul
};
template <bool KMINOR>
__device__ __forceinline__ OperandDev make_operand_dev(const Operand& o) {
    OperandDev d;
    const int64_t n = KMINOR ? (int64_t)o.K * o.ld : (int64_t)o.rows * o.ld;
    d.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(o.ptr), 0, (int)((o.rowmap ? o.nrec : n) * (o.src16 ? 2 : 4)), 0x00020000);
    d.rm = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(o.rowmap ? o.rowmap : reinterpret_cast<const unsigned*>(o.ptr)), 0,
                                             (int)((o.rowmap ? o.map_n : 1) * 4), 0x00020000);
    d.mp = o.rowmap;
    d.bits = o.bits != nullptr;
    d.nomask = d.bits ? 0u : 0xFFFFFFFFu;
    const int64_t nb = (KMINOR ? (int64_t)o.K : (int64_t)o.rows) * o.wpr;
    d.rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(d.bits ? o.bits : reinterpret_cast<const uint32_t*>(o.ptr)), 0,
                                             (int)((d.bits ? nb : 0) * 4), 0x00020000);
    d.ld = (int)o.ld; d.rows = o.rows; d.K = o.K; d.wpr = o.wpr; d.ones_row = o.ones_row;
    return d;
}

// piece q of a tile (q < NQ).  KMAJOR: thread = row tid >> 3 (+ 32 per row pass p), 16-byte k quad tid & 7 (+ 8 h for the
// second half of a 64-wide tile): K tile 64 -> p = q >> 1, h = q & 1; K tile 32 -> p = q, h = 0.  KMINOR: rows 4 (tid & 31)
// .. + 3 of k = 2 (tid >> 5 + 8 p) + h with p = q >> 1, h = q & 1 (K tile 32: p < 2).
template <bool KMINOR, int NP>
__device__ __forceinline__ void piece_ph(int q, int& p, int& h) {
    if (!KMINOR && NP != 1) { p = q; h = 0; }
    else { p = q >> 1; h = q & 1; }
}
// What a thread needs of an operand's block tile at r0 and does not depend on the K tile, computed once per block tile.  Per K
// tile and piece only uniform terms are added (quad_load: one scalar operand; quad_store: immediate LDS offsets).
struct PieceCtx {
    unsigned vb;       // lane byte offset of the thread's pieces: piece 0 of the K tile at k = 0 (K-minor through a row map: its rows only)
    unsigned vr[4];    // K-major through a row map: one lane offset per row pass instead (the map's entries, requested here)
    unsigned wb;       // ... of its mask words
    int lim;           // K-major: rows from the thread's first one to the operand's end (row pass p exists iff 32 p < lim);
                       // K-minor: one bit per row of the piece that exists
    int sh;            // bit of a mask word that belongs to the piece's first element
    int kl;            // K-major: last k of piece 0 inside the K tile; K-minor: its k
    int one;           // K-minor: bit e set iff the piece's row e is the ones row
    int li;            // dword index of piece 0 inside an LDS plane
};
// K-minor operand through its row map: piece q of a thread lies in memory row k = k0 + 2 ((tid >> 5) + 8 p) + h with p = q >> 1,
// h = q & 1, i.e. k0 + 4 wave + 16 p + {0, 1} for the lower half of a wave and + {2, 3} for the upper one: the map entries a
// wave needs for one K tile are KT / 16 aligned groups of four consecutive words, the same for all its lanes.  They are
// requested with SCALAR loads (s_load_dwordx4 through the constant cache) one K tile ahead and turned into the per-lane
// offsets ro[] with one select each -- nothing of the map goes through the vector memory pipe, which is what bounds the
// staging phase of these kernels (as vector loads -- one dword request per piece -- the map cost dW1 14 us of 77).  The map is
// padded with MAP_PAD valid entries behind its last one (Layout::rowmap): requests run up to two K tiles past the K range.
typedef unsigned mapw4 __attribute__((ext_vector_type(4)));
typedef const mapw4 __attribute__((address_space(4)))* map4_ptr;
template <int NP>
struct MapRegs { mapw4 s[Eng<NP>::KT / 16]; };
template <int NP>
__device__ __forceinline__ void map_request(MapRegs<NP>& mr, const OperandDev& o, int k0) {
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x & 255) >> 6);
    const unsigned* base = o.mp + __builtin_amdgcn_readfirstlane(k0) + 4 * wv;
#pragma unroll
    for (int p = 0; p < Eng<NP>::KT / 16; ++p) mr.s[p] = *(map4_ptr)(const void*)(base + 16 * p);
}
template <int NP>
__device__ __forceinline__ void map_offsets(unsigned (&ro)[Eng<NP>::NQ], const MapRegs<NP>& mr) {
    const bool hi = (threadIdx.x & 32) != 0;
#pragma unroll
    for (int q = 0; q < Eng<NP>::NQ; ++q) {
        const int p = q >> 1, h = q & 1;
        ro[q] = hi ? mr.s[p][2 + h] : mr.s[p][h];
    }
}
// IDX: the operand is read through its row map (Operand::rowmap).  K-major: the map entries of the thread's four row passes are
// requested here, once per block tile; K-minor: a new set ro[] per K tile, from map_request / map_offsets above.
template <bool KMINOR, int NP, bool IDX = false>
__device__ __forceinline__ PieceCtx piece_ctx(const OperandDev& o, int r0) {
    const int tid = threadIdx.x & 255;     // (the ping-pong kernels run two 256-thread groups per workgroup)
    PieceCtx c = {};
    if (!KMINOR) {
        const int kq = tid & 7, rr = tid >> 3, row = r0 + rr;
        c.vb = ((unsigned)row * (unsigned)o.ld + kq * 4u) * 4u;
        if constexpr (IDX) {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                c.vr[p] = ((unsigned)__builtin_amdgcn_raw_buffer_load_b32(o.rm, min(row + 32 * p, o.rows - 1) * 4, 0, 0) + kq * 4u) * 4u;
        }
        c.wb = (unsigned)row * (unsigned)o.wpr * 4u;
        c.lim = o.rows - row;
        c.sh = kq * 4;
        c.kl = kq * 4 + 3;
        c.li = rr * Eng<NP>::LDB + kq * 2;
    } else {
        // row % 4 == 0 and ld % 4 == 0: the four floats stay inside the memory row whenever row < rows <= ld
        const int r4 = (tid & 31) * 4, kp = tid >> 5, row = r0 + r4;
        c.vb = IDX ? row * 4u : (2u * kp * (unsigned)o.ld + row) * 4u;
        c.wb = (2u * kp * (unsigned)o.wpr + (row >> 5)) * 4u;
        c.lim = (1 << min(max(o.rows - row, 0), 4)) - 1;
        c.sh = row & 31;
        c.kl = 2 * kp;
        const int e = o.ones_row - row;
        c.one = (o.ones_row >= 0 && e >= 0 && e < 4) ? 1 << e : 0;
        c.li = (2 * kp * Eng<NP>::LDK + r4) >> 1;     // LDK and r4 are multiples of 4 bf16
    }
    return c;
}
// Request piece q of the K tile at k0 (k0 % 32 == 0; kend <= K, kend % 4 == 0).  No branch and no condition around a load: a
// piece either exists entirely or asks for PIECE_OOB.  ro: K-minor through a row map, the element offsets of the pieces' memory rows.
template <bool KMINOR, bool BITS = true, int NP = 1, bool IDX = false>
__device__ __forceinline__ void quad_load(TileRegsT<BITS, Eng<NP>::NQ>& t, const OperandDev& o, const PieceCtx& c, int k0, int kend, int q,
                                          const unsigned* ro = nullptr) {
    int p, h;
    piece_ph<KMINOR, NP>(q, p, h);
    bool ok;
    unsigned vo, so, swo;     // lane offset of the values; uniform terms of the values' and of the mask word's offset
    if (!KMINOR) {
        ok = 32 * p < c.lim && k0 + 32 * h + c.kl < kend;
        vo = IDX ? c.vr[p] : c.vb;
        so = IDX ? (unsigned)(k0 + 32 * h) * 4u : (32u * p * (unsigned)o.ld + k0 + 32 * h) * 4u;
        swo = (32u * p * (unsigned)o.wpr + (k0 >> 5) + h) * 4u;
    } else {
        const int ks = k0 + 16 * p + h;
        ok = c.lim != 0 && ks + c.kl < kend;
        vo = IDX ? ro[q] * 4u + c.vb : c.vb;
        so = IDX ? 0u : (unsigned)ks * (unsigned)o.ld * 4u;
        swo = (unsigned)ks * (unsigned)o.wpr * 4u;
    }
    // (the uniform terms are added to the lane offset and the scalar offset stays 0, as in k_x3_fc11g's request_x: whether the
    // range check adds a scalar offset to the lane offset has not been established for these descriptors, and if it does,
    // PIECE_OOB plus the term wraps back into the range.  This form is right under either rule.)
    t.v[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(o.rs, (int)(ok ? vo + so : PIECE_OOB), 0, 0));
    if constexpr (BITS) t.wd[q] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(o.rb, (int)(ok ? c.wb + swo : PIECE_OOB), 0, 0);
}
// the indexed operand's offsets for its first K tile (and, K-minor, the request for the second one's)
template <bool KMINOR, int NP>
__device__ __forceinline__ void idx_begin(unsigned (&ro)[Eng<NP>::NQ], MapRegs<NP>& mr, const OperandDev& o, int kfirst) {
    if constexpr (KMINOR) {
        map_request<NP>(mr, o, kfirst);
        map_offsets<NP>(ro, mr);
        map_request<NP>(mr, o, kfirst + Eng<NP>::KT);
    }
}
// ... and for the K tile at kld, at the head of the staging phase that requests it
template <bool KMINOR, int NP>
__device__ __forceinline__ void idx_next(unsigned (&ro)[Eng<NP>::NQ], MapRegs<NP>& mr, const OperandDev& o, int kld) {
    if constexpr (KMINOR) {
        map_offsets<NP>(ro, mr);
        map_request<NP>(mr, o, kld + Eng<NP>::KT);
    }
}
// Write piece q of the K tile at k0 to the LDS image.  What does not exist arrived as 0 (quad_load), so only the keep-mask and
// the rows of a K-minor piece beyond the operand are masked here.  BN / ONES (K-minor): the BatchNorm-normalised form and the ones
// row, compiled only where the operand can carry them: k_x3_small's Q (both) and the B operand of the bf16 engine's dW11 forms
// (the fp32x3 GEMMs take their ones column from the slice planes)
template <bool KMINOR, bool BITS = true, int NP = 1, bool BN = false, bool ONES = BN>
__device__ __forceinline__ void quad_store(unsigned* __restrict__ T, const TileRegsT<BITS, Eng<NP>::NQ>& t, const OperandDev& o, const PieceCtx& c,
                                           int k0, int kend, int q) {
    constexpr int PLANE = Eng<NP>::PLANE;
    int p, h;
    piece_ph<KMINOR, NP>(q, p, h);
    const float4 v = t.v[q];
    float x[4] = {v.x, v.y, v.z, v.w};
    int idx;        // dword index of the 8-byte LDS store inside a plane
    if (!KMINOR) {
        // keep bit e of nib -> an all-ones / all-zeros word (v_bfe_i32) ANDed onto the value: two VALU instructions per
        // element and no compare -> SGPR -> select chains
        if constexpr (BITS) {
            const int nib = (int)((t.wd[q] | o.nomask) >> c.sh);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = __uint_as_float(__float_as_uint(x[e]) & (unsigned)__builtin_amdgcn_sbfe(nib, e, 1));
        }
        idx = c.li + 32 * p * Eng<NP>::LDB + 16 * h;
    } else {
        // natural layout [k][row] (rows contiguous, Eng<NP>::LDK bf16 per k): one 8-byte store per (k, four rows); the MFMA
        // fragments come out of it through the transposing LDS read (ds_read_b64_tr_b16, see frag8)
        const int kt = 16 * p + h;
        int nib = BITS ? (int)((t.wd[q] | o.nomask) >> c.sh) & c.lim : c.lim;      // rows of this piece that exist (and are kept)
        int one = c.one;
        if constexpr (ONES) {       // a k that does not exist stays 0 under these forms too
            const bool kok = k0 + kt + c.kl < kend;
            nib = kok ? nib : 0;
            one = kok ? one : 0;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned m = (unsigned)__builtin_amdgcn_sbfe(nib, e, 1);
            if constexpr (BN) {     // BatchNorm-normalised input, as k_gemm_tn: (v - mean) * rstd; rows / k that do not exist stay 0
                const float sb[4] = {o.bn_sub.x, o.bn_sub.y, o.bn_sub.z, o.bn_sub.w}, ml[4] = {o.bn_mul.x, o.bn_mul.y, o.bn_mul.z, o.bn_mul.w};
                x[e] = __uint_as_float(__float_as_uint((x[e] - sb[e]) * ml[e]) & m);
            } else x[e] = __uint_as_float(__float_as_uint(x[e]) & m);
            if constexpr (ONES) {
                const unsigned m1 = (unsigned)__builtin_amdgcn_sbfe(one, e, 1);
                x[e] = __uint_as_float((__float_as_uint(x[e]) & ~m1) | (__float_as_uint(1.f) & m1));
            }
        }
        idx = c.li + ((kt * Eng<NP>::LDK) >> 1);
    }
    if constexpr (NP == 1) {
        uint2 w;
        w.x = pack_bf16(x[0], x[1]);
        w.y = pack_bf16(x[2], x[3]);
        *reinterpret_cast<uint2*>(&T[idx]) = w;
    } else {
        unsigned w0[3], w1[3];
        split3(x[0], x[1], w0);
        split3(x[2], x[3], w1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<uint2*>(&T[pl * PLANE + idx]) = make_uint2(w0[pl], w1[pl]);
    }
}

// ---- operands kept as bf16 in HBM (Operand::src16; one-plane engine, K tile 64) ----------------------------------------------
// A piece is 16 bytes = EIGHT elements, four pieces per thread and K tile (an fp32 operand: eight pieces of four): K-major
// piece p = row (tid >> 3) + 32 p, k = k0 + 8 (tid & 7) .. + 7; K-minor piece p = memory row k = k0 + (tid >> 4) + 16 p, rows
// 8 (tid & 15) .. + 7.  The values are what quad_store would have produced from the fp32 original (round to nearest even, at
// the producer instead of here), so they go to the LDS image as they are -- one 16-byte store, no conversion -- with the keep
// bits ANDed on as half-word masks.  IDX: through the row map; ro[p] is the element offset of piece p's memory row.
struct OctRegs { u32x4v v[4]; uint32_t wd[4]; };
template <bool KMINOR, bool IDX>
__device__ __forceinline__ void oct_load(OctRegs& t, const OperandDev& o, int r0, int k0, int kend, int p, const unsigned (&ro)[8]) {
    const int tid = threadIdx.x & 255;
    int off, woff;
    if (!KMINOR) {
        const int row = r0 + (tid >> 3) + 32 * p;
        const int rc = min(row, o.rows - 1);
        const int k = k0 + 8 * (tid & 7);
        const bool ok = row < o.rows && k + 7 < kend && k + 7 < o.K;         // K % 8 == 0, k0 % 8 == 0
        off = (IDX ? (int)ro[p] : rc * o.ld) + (ok ? k : 0);
        woff = rc * o.wpr + ((ok ? k : 0) >> 5);
    } else {
        const int k = k0 + (tid >> 4) + 16 * p;
        const int kc = min(k, o.K - 1);
        const int row = r0 + 8 * (tid & 15);                                 // ld % 8 == 0: the eight stay inside the memory row
        off = (IDX ? (int)ro[p] : kc * o.ld) + (row < o.ld ? row : 0);
        woff = kc * o.wpr + (min(row, o.rows - 1) >> 5);
    }
    t.v[p] = __builtin_bit_cast(u32x4v, __builtin_amdgcn_raw_buffer_load_b128(o.rs, off * 2, 0, 0));
    t.wd[p] = o.bits ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(o.rb, woff * 4, 0, 0) : 0xFFFFFFFFu;
}
template <bool KMINOR>
__device__ __forceinline__ void oct_store(unsigned* __restrict__ T, const OctRegs& t, const OperandDev& o, int r0, int k0, int kend, int p) {
    const int tid = threadIdx.x & 255;
    int byte, idx;      // keep bits of the eight elements; dword index of the 16-byte LDS store
    if (!KMINOR) {
        const int rr = (tid >> 3) + 32 * p, row = r0 + rr;
        const int k = k0 + 8 * (tid & 7);
        const bool ok = row < o.rows && k + 7 < kend && k + 7 < o.K;
        byte = ok ? (int)((t.wd[p] >> (k & 31)) & 0xFFu) : 0;
        idx = rr * LDB + 4 * (tid & 7);
    } else {
        const int kl = (tid >> 4) + 16 * p, k = k0 + kl;
        const int r8 = 8 * (tid & 15);
        const bool kok = k < kend && k < o.K;
        const int nrow = min(max(o.rows - (r0 + r8), 0), 8);
        byte = kok ? (int)((t.wd[p] >> ((r0 + r8) & 31)) & ((1u << nrow) - 1u)) : 0;
        idx = (kl * LDK + r8) >> 1;
    }
    u32x4v w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned m = ((unsigned)__builtin_amdgcn_sbfe(byte, 2 * j, 1) & 0xFFFFu) | ((unsigned)__builtin_amdgcn_sbfe(byte, 2 * j + 1, 1) & 0xFFFF0000u);
        w[j] = t.v[p][j] & m;
    }
    *reinterpret_cast<u32x4v*>(&T[idx]) = w;
}
// row-map offsets of the four pieces: K-major once per block tile; K-minor per K tile from the scalar map registers (the
// memory rows of a wave's pieces are k0 + 4 wave + 16 p + quarter-wave: the same groups of four words as map_request reads)
__device__ __forceinline__ void oct_ro_init(unsigned (&ro)[8], const OperandDev& o, int r0) {
    const int tid = threadIdx.x & 255;
#pragma unroll
    for (int p = 0; p < 4; ++p) ro[p] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(o.rm, min(r0 + (tid >> 3) + 32 * p, o.rows - 1) * 4, 0, 0);
}
__device__ __forceinline__ void oct_map_offsets(unsigned (&ro)[8], const MapRegs<1>& mr) {
    const int qq = (threadIdx.x >> 4) & 3;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const unsigned lo = (qq & 1) ? mr.s[p][1] : mr.s[p][0], hi = (qq & 1) ? mr.s[p][3] : mr.s[p][2];
        ro[p] = (qq & 2) ? hi : lo;
    }
}

template <bool KMINOR, bool BITS = true, int NP = 1>
__device__ __forceinline__ void tile_load(TileRegsT<BITS, Eng<NP>::NQ>& t, const OperandDev& o, int r0, int k0, int kend) {
    const PieceCtx c = piece_ctx<KMINOR, NP>(o, r0);
#pragma unroll
    for (int q = 0; q < Eng<NP>::NQ; ++q) quad_load<KMINOR, BITS, NP>(t, o, c, k0, kend, q);
}
template <bool KMINOR, bool BITS = true, int NP = 1>
__device__ __forceinline__ void tile_store(unsigned* __restrict__ T, const TileRegsT<BITS, Eng<NP>::NQ>& t, const OperandDev& o, int r0,
                                           int k0, int kend) {
    const PieceCtx c = piece_ctx<KMINOR, NP>(o, r0);
#pragma unroll
    for (int q = 0; q < Eng<NP>::NQ; ++q) quad_store<KMINOR, BITS, NP>(T, t, o, c, k0, kend, q);
}

// MFMA fragment of a 32-row tile (rows rb .. rb + 31 of the block tile), K step s (16 k's): lane l holds row l % 32,
// k = 16 s + 8 (l / 32) .. + 7.  KMAJOR image: one ds_read_b128.  KMINOR image ([k][row]): two transposing reads -- per
// group of 16 lanes the hardware reads a 4 (k) x 16 (rows) block and hands lane i of the group column i, i.e. four
// consecutive k of row i; lane 4 q + p supplies the address of block row q, columns 4 p .. 4 p + 3.
typedef short s16x4 __attribute__((ext_vector_type(4)));
template <bool MINOR, int LDBv = LDB, int LDKv = LDK>
__device__ __forceinline__ bf16x8 frag8(const unsigned* T, int rb, int s, int lane) {
    if (!MINOR) {
        return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(T + (rb + (lane & 31)) * LDBv + 4 * (lane >> 5) + 8 * s));
    } else {
        const unsigned short* Tk = reinterpret_cast<const unsigned short*>(T);
        const int grp = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
        const unsigned short* a = Tk + (16 * s + 8 * (grp >> 1) + q) * LDKv + rb + 16 * (grp & 1) + 4 * p;
        typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)a);
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 4 * LDKv));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        s16x8 r;
        r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
        r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
        return __builtin_bit_cast(bf16x8, r);
    }
}

// A K tile of an operand that exists as slice planes: 3 planes x 128 x 32 bf16 = 1536 sixteen-byte pieces, six per thread
// of a 256-thread group; a piece is copied global -> register -> LDS untouched (no bounds, no arithmetic).
struct PlaneRegs { u32x4v v[6]; };
struct PlaneDev { __amdgpu_buffer_rsrc_t rs; int plane, ld; };
__device__ __forceinline__ PlaneDev make_plane_dev(const Operand& o, int arm) {
    PlaneDev d;
    d.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(o.pl + (int64_t)arm * o.pl_arm), 0, (int)(3 * o.pl_plane * 2), 0x00020000);
    d.plane = (int)o.pl_plane; d.ld = o.pl_ld;
    return d;
}
template <bool KMINOR>
__device__ __forceinline__ void plane_load(PlaneRegs& t, const PlaneDev& o, int r0, int k0, int j) {
    // piece id = tid + 256 (j & 1) of plane j >> 1.  The lane offset is the thread's own (the same for every piece and K tile);
    // plane, tile origin, K tile and the piece's half ride in the scalar offset (the planes are padded: no bounds)
    const int tid = threadIdx.x & 255, pl = j >> 1, hi = j & 1;
    int vo, so;   // elements
    if (!KMINOR) { vo = (tid >> 2) * o.ld + 8 * (tid & 3); so = pl * o.plane + (r0 + 64 * hi) * o.ld + k0; }      // row id >> 2, k octet id & 3
    else { vo = (tid >> 4) * o.ld + 8 * (tid & 15); so = pl * o.plane + (k0 + 16 * hi) * o.ld + r0; }             // k id >> 4, row octet id & 15
    t.v[j] = __builtin_bit_cast(u32x4v, __builtin_amdgcn_raw_buffer_load_b128(o.rs, vo * 2, so * 2, 0));
}
template <bool KMINOR>
__device__ __forceinline__ void plane_store(unsigned* __restrict__ T, const PlaneRegs& t, int j) {
    const int tid = threadIdx.x & 255, pl = j >> 1, id = tid + 256 * (j & 1);
    int idx;   // dwords
    if (!KMINOR) idx = pl * Eng<3>::PLANE + (id >> 2) * Eng<3>::LDB + 4 * (id & 3);
    else idx = pl * Eng<3>::PLANE + (((id >> 4) * Eng<3>::LDK + 8 * (id & 15)) >> 1);
    *reinterpret_cast<u32x4v*>(&T[idx]) = t.v[j];
}

// fp32 [R][C] (row pitch ld) -> three bf16 slice planes [3][Rp][Cp], zeros outside, column `ones_col` reads 1.0 on the
// rows that exist (the bias-gradient column of [d10 | 1]).  One thread: eight consecutive columns of one row.
struct SplitJob {
    const float* src; int64_t ld, src_arm;
    int R, C, Rp, Cp, ones_col;
    unsigned short* dst; int64_t dst_arm;
    const float* col_src; int64_t col_arm;   // column `ones_col` reads col_src[row] instead of 1.0 (the bias column of [W11 | b11])
    int tr;                                  // 1: the planes hold the TRANSPOSE -- element (r, c) = src[c * ld + r]; R, C are the planes' extents
};
// The head of a training step as one launch: besides the split jobs, the first xb.blocks blocks of every z-slice make the
// dropout keep-mask (k_make_xbits' work) and the whole grid zeroes the step's loss partial slots and forward accumulator
// sets -- one launch boundary and one tail less on the critical path.
struct XbitsJob {
    NoiseDev nz; int A, B, D, wpr; uint32_t* bits; int blocks; float* zero_p; int zero_n4;
    // mmvae_train_step_rows: the row map of the batch, map[b] = rows[b] * ld (element offset of cell b's row in the resident
    // matrix; indices outside [0, n_rows) are clamped as mmvae_gather_rows does) -- null: the batch is materialised
    const int64_t* rows; unsigned* map; int64_t rows_ld, n_rows;
};
struct SplitJobs { SplitJob j[24]; int first[25]; int n; XbitsJob xb; };   // job i owns blocks [first[i], first[i + 1]) of grid.x (behind xb.blocks)
__global__ __launch_bounds__(256) void k_presplit(const SplitJobs js) {
    if (js.xb.zero_n4 > 0) grid_zero(js.xb.zero_p, js.xb.zero_n4);
    if (js.xb.rows && blockIdx.z == 0) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < js.xb.B + MAP_PAD; i += gridDim.x * 256) {   // the pad reads row 0
            const int64_t r = i < js.xb.B ? js.xb.rows[i] : 0;
            js.xb.map[i] = (unsigned)((r < 0 ? 0 : (r >= js.xb.n_rows ? js.xb.n_rows - 1 : r)) * js.xb.rows_ld);
        }
    }
    if ((int)blockIdx.x < js.xb.blocks) {
        make_xbits_range(js.xb.nz, js.xb.A, js.xb.B, js.xb.D, js.xb.wpr, js.xb.bits,
                         ((int64_t)blockIdx.z * js.xb.blocks + blockIdx.x) * 256 + threadIdx.x, (int64_t)gridDim.z * js.xb.blocks * 256);
        return;
    }
    const int bx0 = (int)blockIdx.x - js.xb.blocks;
    int ji = 0;
    while (ji + 1 < js.n && bx0 >= js.first[ji + 1]) ++ji;
    const SplitJob& J = js.j[ji];
    const int bx = bx0 - js.first[ji], nbx = js.first[ji + 1] - js.first[ji];
    const float* src = J.src + (int64_t)blockIdx.z * J.src_arm;
    const float* col = J.col_src ? J.col_src + (int64_t)blockIdx.z * J.col_arm : nullptr;
    unsigned short* dst = J.dst + (int64_t)blockIdx.z * J.dst_arm;
    const int c8n = J.Cp >> 3;                      // eight-column pieces per row
    const int64_t plane = (int64_t)J.Rp * J.Cp;
    const bool vec = (J.ld & 3) == 0 && (J.C & 3) == 0;
    // a thread keeps its piece column and walks the rows (row pitch of the walk: 256 / c8n rows when c8n <= 256)
    const int n = J.Rp * c8n;
    for (int i = bx * 256 + threadIdx.x; i < n; i += nbx * 256) {
        const int r = i / c8n, c0 = (i - r * c8n) * 8;
        float v[8];
        if (J.tr) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (r < J.R && c0 + e < J.C) ? src[(int64_t)(c0 + e) * J.ld + r] : 0.f;
        } else if (r < J.R && vec && c0 + 8 <= J.C) {
            const float4 a = *reinterpret_cast<const float4*>(src + (int64_t)r * J.ld + c0);
            const float4 b = *reinterpret_cast<const float4*>(src + (int64_t)r * J.ld + c0 + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = c0 + e;
                v[e] = (r < J.R && c < J.C) ? src[(int64_t)r * J.ld + c] : ((r < J.R && c == J.ones_col) ? (col ? col[r] : 1.f) : 0.f);
            }
        }
        unsigned w[4][3];
#pragma unroll
        for (int e = 0; e < 4; ++e) split3(v[2 * e], v[2 * e + 1], w[e]);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(dst + pl * plane + (int64_t)r * J.Cp + c0) = make_uint4(w[0][pl], w[1][pl], w[2][pl], w[3][pl]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// epilogues
// ---------------------------------------------------------------------------------------------------------------
struct SlabOut {       // C tile -> out[(ks * A + arm)][m][n], m < M, n < N
    float* out;
    int64_t ks_stride, arm_stride;
    int ld, M, N;
};
struct Fc11Out {       // z tile -> + bias, dZ11, loss partials (nn_model.py:286, :542-546 and their autograd)
    const float* bias; // [D], arm stride bias_arm
    const float* x;    // this arm's [B][D]
    float* dz;         // this arm's [B][D]
    float* x_rec;      // this arm's [B][D] or null
    float* part;       // this arm's loss partial slots [n11][2]
    float coef;
    int B, D;
    const unsigned* xmap;   // row indirection (k_x3_fc11g): cell b's row of x lies at x[xmap[b] ..), x_nrec floats addressable; null: x[b * D ..)
    int64_t x_nrec;
};

struct GemmArgs {
    Operand a, b;
    int64_t a_arm, b_arm;        // arm strides of the operands (floats); mask bits: a_bits_arm / b_bits_arm (words)
    int64_t a_bits_arm, b_bits_arm;
    int64_t bias_arm;            // arm stride of fo.bias
    int M, N, K;
    int KS;                      // splits of the k range (grid.y) -- or of the n tiles when loop_n
    SlabOut so;
    Fc11Out fo;
    int64_t fo_arm, fo_x_arm;    // arm strides of dz / x_rec and of x (0: the arms share x)
    int n11;
    int A;
};

// the MFMAs of one K tile: this wave's 64 x 64 of the block tile (NP = 3: six slice products per pair of fragments, the
// small ones first)
template <bool AMINOR, bool BMINOR, int NP = 1>
__device__ __forceinline__ void mfma_ktile(f32x16 (&acc)[2][2], const unsigned* As, const unsigned* Bs, int wm, int wn, int lane) {
    constexpr int LDBv = Eng<NP>::LDB, PLANE = Eng<NP>::PLANE, NS = Eng<NP>::KT / 16;
    // NP = 3: the K tile has two K steps; the fragments of the second are requested before the MFMAs of the first (a
    // ds_read that is waited for at once costs 64+ cycles -- tools/micro/x3_issue_bench.hip -- and hipcc sinks reads
    // towards their uses: the fence keeps them where they are)
    bf16x8 a[NP == 3 ? 2 : 1][2][NP], b[NP == 3 ? 2 : 1][2][NP];
    auto frags = [&](int s, int w) __attribute__((always_inline)) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
            a[w][0][pl] = frag8<AMINOR, LDBv, Eng<NP>::LDK>(As + pl * PLANE, wm * 64, s, lane);
            a[w][1][pl] = frag8<AMINOR, LDBv, Eng<NP>::LDK>(As + pl * PLANE, wm * 64 + 32, s, lane);
            b[w][0][pl] = frag8<BMINOR, LDBv, Eng<NP>::LDK>(Bs + pl * PLANE, wn * 64, s, lane);
            b[w][1][pl] = frag8<BMINOR, LDBv, Eng<NP>::LDK>(Bs + pl * PLANE, wn * 64 + 32, s, lane);
        }
    };
    if constexpr (NP == 3) {
        frags(0, 0);
        frags(1, 1);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int w = NP == 3 ? s : 0;
        if constexpr (NP != 3) frags(s, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if constexpr (NP == 3) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][2], b[w][j][0], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][0], b[w][j][2], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][1], b[w][j][1], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][1], b[w][j][0], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][0], b[w][j][1], acc[i][j], 0, 0, 0);
                }
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[w][i][0], b[w][j][0], acc[i][j], 0, 0, 0);
            }
    }
}

// The tile epilogue: accumulator register r of tile (i, j) is row m0 + 64 wm + 32 i + acc_row(r), column
// n0 + 64 wn + 32 j + (lane & 31) of out[M][N] (row pitch ld).  One buffer descriptor per block: it starts at the tile's first
// row and its range ends with the last row that exists, so rows beyond M are dropped by the hardware, and a lane whose column
// lies beyond N asks for an offset past every range -- no branch and no 64-bit address per element.  The whole offset is the
// per-lane one and the scalar offset is 0, so the range check sees all of it.  128 ld floats stay far below TILE_OOB.
constexpr unsigned TILE_OOB = 0x80000000u;
__device__ __forceinline__ void tile_out(float* out, int ld, int M, int N, const f32x16 (&acc)[2][2], int m0, int n0, int wm, int wn, int lane) {
    // (uniform, but hipcc forms the clamp on the vector unit: a descriptor in VGPRs would cost every store a waterfall loop)
    const int rows = __builtin_amdgcn_readfirstlane(min(max(M - m0, 0), BT));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out + (int64_t)m0 * ld, 0, rows * ld * 4, 0x00020000);
    const unsigned ldb = (unsigned)ld * 4u;
    const unsigned row_l = (unsigned)(64 * wm + 4 * (lane >> 5)) * ldb;      // the lane's part of its accumulator rows (acc_row)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + 64 * wn + 32 * j + (lane & 31);
        const unsigned o_lane = col < N ? row_l + (unsigned)col * 4u : TILE_OOB;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = acc[i][j][r];      // (a copy: __builtin_bit_cast of the vector ELEMENT reads element 0)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)(o_lane + (unsigned)(32 * i + acc_row(r, 0)) * ldb), 0, 0);
            }
    }
}
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, const f32x16 (&acc)[2][2], int m0, int n0, int wm, int wn, int lane, int arm) {
    tile_out(g.so.out + (int64_t)blockIdx.y * g.so.ks_stride + (int64_t)arm * g.so.arm_stride, g.so.ld, g.so.M, g.so.N, acc, m0, n0, wm, wn, lane);
}

// C tile -> slab.  grid (tiles_m * tiles_n, KS, A): block (m tile, n tile) x k range ks x arm.  Tile t + 1 is written to
// the second LDS buffer while tile t is multiplied (one barrier per K tile); a piece's registers request tile t + 2 as
// soon as they have been written out for tile t + 1.
// IDX: 1 / 2 = the A / B operand through its row map (see k_x3_gemm); S16: bit 0 / bit 1 = the A / B operand is bf16 in memory
// XMASK: x~ -- fc1's A, dW1's B -- may carry its keep-mask (a null mask then reads as all ones: OperandDev::nomask); the forms
// without it request no mask words at all (as out-of-range requests they cost dW11 on a bf16 dZ11 10 us of 105)
template <bool AMINOR, bool BMINOR, int IDX = 0, int S16 = 0, bool XMASK = true>
__global__ __launch_bounds__(256, 2) void k_bf16_gemm(const GemmArgs g_in) {
    const GemmArgs g = g_in;
    __shared__ __attribute__((aligned(16))) unsigned As[2][BT * LDB];   // two K tiles in LDS: tile t is multiplied while tile
    __shared__ __attribute__((aligned(16))) unsigned Bs[2][BT * LDB];   // t + 1 is written and tile t + 2 is in flight
    const int arm = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    Operand oa_h = g.a, ob_h = g.b;
    oa_h.ptr += (int64_t)arm * g.a_arm;
    ob_h.ptr += (int64_t)arm * g.b_arm;
    if (oa_h.bits) oa_h.bits += (int64_t)arm * g.a_bits_arm;
    if (ob_h.bits) ob_h.bits += (int64_t)arm * g.b_bits_arm;
    const OperandDev oa = make_operand_dev<AMINOR>(oa_h), ob = make_operand_dev<BMINOR>(ob_h);
    const int tiles_n = cdiv(g.N, BT);
    const int wg = blockIdx.x;
    const int m0 = (wg / tiles_n) * BT, n0 = (wg % tiles_n) * BT;
    const int nkt = cdiv(g.K, KT);
    const int kb = (int)(((int64_t)blockIdx.y * nkt) / g.KS) * KT;
    const int ke = min(g.K, (int)(((int64_t)(blockIdx.y + 1) * nkt) / g.KS) * KT);
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    constexpr bool ABITS = XMASK && !AMINOR && !BMINOR, BBITS = XMASK && AMINOR && BMINOR;
    TileRegsT<ABITS> ta;
    TileRegsT<BBITS> tb;
    OctRegs t16a, t16b;                // S16 (bit 0: A, bit 1: B): a bf16-source operand's pieces (ta / tb of that operand stay unused)
    unsigned ro[Eng<1>::NQ] = {};      // IDX: element offsets of the indexed operand's memory rows (K-minor fp32 pieces: quad_load; bf16 pieces: oct_load)
    MapRegs<1> mr = {};
    static_assert(IDX == 0 || S16 == 0 || (S16 & IDX) != 0, "row map and bf16 storage: the indexed operand (x) is a bf16 one");
    constexpr bool A16 = (S16 & 1) != 0, B16 = (S16 & 2) != 0;
    constexpr bool AIDX = IDX == 1 && !A16, BIDX = IDX == 2 && !B16;     // through the row map as fp32 pieces
    constexpr bool BONES = AMINOR && BMINOR && IDX == 0;                  // B may carry a ones row: the dW11 forms (launch_slab_gemm checks)
    const PieceCtx ca = piece_ctx<AMINOR, 1, AIDX>(oa, m0), cb = piece_ctx<BMINOR, 1, BIDX>(ob, n0);
    // Software pipeline at the granularity of one 16-byte piece: a piece of tile t + 1 is rounded and written to LDS
    // and the SAME registers immediately request the piece of tile t + 2, so sixteen loads per thread are in flight
    // all the time and every load has a whole iteration (the other fifteen pieces, the MFMAs, the barrier) to land.
    auto stage = [&](unsigned* Ad, unsigned* Bd, int kst, int kld, auto load_tag) __attribute__((always_inline)) {
        constexpr bool LOAD = decltype(load_tag)::value;
        if constexpr (LOAD && IDX == 1 && AMINOR) {
            if constexpr (A16) { oct_map_offsets(ro, mr); map_request<1>(mr, oa, kld + KT); }
            else idx_next<AMINOR, 1>(ro, mr, oa, kld);
        }
        if constexpr (LOAD && IDX == 2 && BMINOR) {
            if constexpr (B16) { oct_map_offsets(ro, mr); map_request<1>(mr, ob, kld + KT); }
            else idx_next<BMINOR, 1>(ro, mr, ob, kld);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            // (no run-time condition around a load: hipcc then waits for every load separately)
            if constexpr (A16) {
                if (q < 4) {
                    oct_store<AMINOR>(Ad, t16a, oa, m0, kst, ke, q);
                    if constexpr (LOAD) oct_load<AMINOR, IDX == 1>(t16a, oa, m0, kld, ke, q, ro);
                }
            } else {
                quad_store<AMINOR, ABITS>(Ad, ta, oa, ca, kst, ke, q);
                if constexpr (LOAD) quad_load<AMINOR, ABITS, 1, AIDX>(ta, oa, ca, kld, ke, q, ro);
            }
            if constexpr (B16) {
                if (q < 4) {
                    oct_store<BMINOR>(Bd, t16b, ob, n0, kst, ke, q);
                    if constexpr (LOAD) oct_load<BMINOR, IDX == 2>(t16b, ob, n0, kld, ke, q, ro);
                }
            } else {
                quad_store<BMINOR, BBITS, 1, false, BONES>(Bd, tb, ob, cb, kst, ke, q);
                if constexpr (LOAD) quad_load<BMINOR, BBITS, 1, BIDX>(tb, ob, cb, kld, ke, q, ro);
            }
        }
    };
    // first K tile: the indexed operand's offsets, then every piece's request
    auto first = [&](auto a_tag) __attribute__((always_inline)) {
        constexpr bool ISA = decltype(a_tag)::value;
        constexpr bool MINOR = ISA ? AMINOR : BMINOR;
        constexpr bool IDXD = IDX == (ISA ? 1 : 2), IS16 = ISA ? A16 : B16;
        const OperandDev& o = ISA ? oa : ob;
        const int r0 = ISA ? m0 : n0;
        OctRegs& t16 = ISA ? t16a : t16b;
        if constexpr (IS16) {
            if constexpr (IDXD) {
                if constexpr (MINOR) { map_request<1>(mr, o, kb); oct_map_offsets(ro, mr); map_request<1>(mr, o, kb + KT); }
                else oct_ro_init(ro, o, r0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) oct_load<MINOR, IDXD>(t16, o, r0, kb, ke, q, ro);
        } else {
            if constexpr (IDXD) idx_begin<MINOR, 1>(ro, mr, o, kb);
#pragma unroll
            for (int q = 0; q < Eng<1>::NQ; ++q) {
                if constexpr (ISA) quad_load<MINOR, ABITS, 1, IDXD>(ta, o, ca, kb, ke, q, ro);
                else quad_load<MINOR, BBITS, 1, IDXD>(tb, o, cb, kb, ke, q, ro);
            }
        }
    };
    if (kb < ke) {
        first(VecTag{});
        first(ScalarTag{});
    }
    if (kb < ke) {
        if (kb + KT < ke) stage(As[0], Bs[0], kb, kb + KT, VecTag{});
        else stage(As[0], Bs[0], kb, kb, ScalarTag{});
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = kb; k0 < ke; k0 += KT) {
        mfma_ktile<AMINOR, BMINOR>(acc, As[cur], Bs[cur], wm, wn, lane);
        if (k0 + 2 * KT < ke) stage(As[cur ^ 1], Bs[cur ^ 1], k0 + KT, k0 + 2 * KT, VecTag{});
        else if (k0 + KT < ke) stage(As[cur ^ 1], Bs[cur ^ 1], k0 + KT, k0 + KT, ScalarTag{});
        __syncthreads();
        cur ^= 1;
    }
    gemm_epilogue(g, acc, m0, n0, wm, wn, lane, arm);
}

// The split (NP = 3) engine: fp32 operands as three bf16 planes each, six MFMAs per pair of fragments.  With six times the
// matrix instructions and eleven VALU instructions per pair of elements for the split, a block tile is no longer a pure
// memory stream: the matrix phase (48 MFMAs per wave and K tile of 32) and the staging phase (split + LDS writes + the
// next requests) are about equally long, and two independent workgroups per CU did not overlap them (measured: the sum of
// the phases, 93 us for fc1).  So ONE workgroup of 512 threads carries TWO block tiles in lock-step ping-pong: group 0
// (waves 0-3) multiplies its K tile t while group 1 (waves 4-7, one per SIMD beside a wave of group 0) stages its own,
// and at every workgroup barrier the roles swap -- each SIMD always has one wave on the matrix pipe and one on the
// VALU / LDS / memory pipes.  A group owns one LDS buffer set (3 planes x 2 operands x 10 KB = 60 KB; 120 KB per CU).
// grid (ceil(tiles / 2), KS, A): group g of block b owns tile 2 b + g.
// SHARE: the two tiles of a block are neighbours along m when the GEMM is one tile wide (fc1, d(d10), dW11: same n0,
// SHARE = 2) or along n when it is one tile high (dW1: same m0, SHARE = 1) -- the narrow operand's K tile is then the
// SAME for both groups, and what bounds these kernels is the bytes a CU takes in (about 13 B per cycle, measured with
// in-kernel stamps: a stage phase lasts as long as its loads take to issue).  Group 0 stages the shared operand for both
// (two LDS buffers, indexed by the K tile's parity; group 1 multiplies tile t while group 0 already stages tile t + 1), a
// quarter less traffic per pair of tiles.  LDS: two private + two shared buffer sets of 30 KB = 120 KB.
// The shared operand comes as slice planes (k_presplit, or the kernel that produced it) and is copied, not split again by
// every block.
// IDX: 1 / 2 = the A / B operand is read through its row map (Operand::rowmap: x of a batch that is never materialised)
// K tiles of the fp32 operand a group keeps in flight.  2 (-DX3_DEPTH=2) was measured and lost: the kernels sit at 234 - 242 of
// the 256 registers a thread of a 512-thread workgroup has, twenty more for the second tile spilled (2 - 40 registers) and
// stretched the schedule -- fc1 79 -> 123 us, dW1 80 -> 108 us
#ifndef X3_DEPTH
#define X3_DEPTH 1
#endif
static_assert(X3_DEPTH == 1 || X3_DEPTH == 2, "one or two K tiles in flight");
// MASK: the fp32 operand carries a keep-mask (known at launch: a kernel without it requests no mask words at all)
template <bool AMINOR, bool BMINOR, int SHARE, int IDX = 0, bool MASK = true>
__global__ __launch_bounds__(512, 1) void k_x3_gemm(const GemmArgs g_in) {
    static_assert(SHARE == 1 || SHARE == 2, "the two tiles of a block share one operand");
    static_assert(IDX == 0 || IDX == (SHARE == 2 ? 1 : 2), "the row map belongs to the operand that is read as fp32");
    typedef Eng<3> E;
    constexpr int KTv = E::KT;
    // F: the operand a group reads as fp32 and splits itself; P: the one both tiles share, copied from its slice planes
    constexpr bool FMINOR = SHARE == 2 ? AMINOR : BMINOR, PMINOR = SHARE == 2 ? BMINOR : AMINOR, IDXD = IDX != 0;
    const GemmArgs g = g_in;
    __shared__ __attribute__((aligned(16))) unsigned As[2][3 * E::PLANE];
    __shared__ __attribute__((aligned(16))) unsigned Bs[2][3 * E::PLANE];
    // the group index as a SCALAR: what follows from it -- the tile, whether it exists, which operands the group stages, the LDS
    // buffers -- is then decided by scalar branches, and no load or LDS store of the steps sits in an exec-masked region
    const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    const int arm = blockIdx.z, tid = threadIdx.x & 255, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    Operand of_h = SHARE == 2 ? g.a : g.b;
    of_h.ptr += (int64_t)arm * (SHARE == 2 ? g.a_arm : g.b_arm);
    if (of_h.bits) of_h.bits += (int64_t)arm * (SHARE == 2 ? g.a_bits_arm : g.b_bits_arm);
    const OperandDev of = make_operand_dev<FMINOR>(of_h);
    // The two tiles of a block: neighbours along m for the same n tile when they share the B operand (SHARE = 2), along n
    // for the same m tile when they share A (SHARE = 1).  An odd count leaves the last block's second group idle.
    const int tiles_m = cdiv(g.M, BT), tiles_n = cdiv(g.N, BT);
    const int bi = blockIdx.x;
    int tm, tn;
    if (SHARE == 2) { tn = bi % tiles_n; tm = 2 * (bi / tiles_n) + grp; }
    else { tm = bi % tiles_m; tn = 2 * (bi / tiles_m) + grp; }
    const bool active = tm < tiles_m && tn < tiles_n;
    const int m0 = tm * BT, n0 = tn * BT;
    const int rf = SHARE == 2 ? m0 : n0, rp = SHARE == 2 ? n0 : m0;      // tile origins of F and P
    const int nkt = cdiv(g.K, KTv);
    const int kb = (int)(((int64_t)blockIdx.y * nkt) / g.KS) * KTv;
    const int ke = min(g.K, (int)(((int64_t)(blockIdx.y + 1) * nkt) / g.KS) * KTv);
    const int n = ke > kb ? cdiv(ke - kb, KTv) : 0;  // K tiles of this block
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    // X3_DEPTH K tiles of a group's fp32 operand are in flight (register slot = tile index % X3_DEPTH).  With one, a CU keeps
    // about 30 KB in flight and takes in 26 GB/s -- the latency-bound part of the intake curve (tools/micro/intake_bench.hip,
    // profiles/r03_intake_microbench.txt: 29 GB/s at 16 KB in flight, 46 at 32 - 64 KB from L2, 28 from HBM) --, but the second
    // tile's registers are not there (see X3_DEPTH above)
    constexpr int DEPTH = X3_DEPTH;
    // (only the fp32 operand -- the one that comes from HBM -- goes two deep: twenty registers; with the slice planes two deep
    // as well the kernel spilled 48 - 64 registers)
    TileRegsT<MASK, E::NQ> tf_[DEPTH];
    unsigned ro[E::NQ] = {};           // K-minor through the row map: element offsets of the pieces' memory rows (see quad_load)
    MapRegs<3> mr = {};
    PlaneRegs ps;
    const PlaneDev dp = make_plane_dev(SHARE == 1 ? g.a : g.b, arm);
    const PieceCtx cf = piece_ctx<FMINOR, 3, IDXD>(of, rf);
    // one piece of each operand in turn; a piece's registers request the next tile as soon as they have been written out
    // kst: the tile whose registers (slot SLOT) are written out; kld: the tile they then request (DEPTH tiles on, LOAD); kpl:
    // the tile the plane registers request (one tile on, LOADP).  Group 0 stages the shared operand, for both groups: a scalar
    // branch around its pieces, since the group index is a scalar
    auto stage = [&](unsigned* Fd, unsigned* Pd, int kst, int kld, int kpl, auto load_tag, auto loadp_tag, auto slot_tag) __attribute__((always_inline)) {
        constexpr bool LOAD = decltype(load_tag)::value, LOADP = decltype(loadp_tag)::value;
        constexpr int SLOT = decltype(slot_tag)::value;
        TileRegsT<MASK, E::NQ>& tf = tf_[SLOT];
        if constexpr (LOAD && IDXD) idx_next<FMINOR, 3>(ro, mr, of, kld);
        auto planes = [&](int i) __attribute__((always_inline)) {
            if (grp == 0) {
                plane_store<PMINOR>(Pd, ps, i);
                if constexpr (LOADP) plane_load<PMINOR>(ps, dp, rp, kpl, i);
            }
        };
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if constexpr (SHARE == 1) planes(i);      // (A before B)
            if (i < E::NQ) {
                quad_store<FMINOR, MASK, 3>(Fd, tf, of, cf, kst, ke, i);
                if constexpr (LOAD) quad_load<FMINOR, MASK, 3, IDXD>(tf, of, cf, kld, ke, i, ro);
            }
            if constexpr (SHARE == 2) planes(i);
        }
    };
    // the first DEPTH tiles' requests (tile d into slot d)
    auto first = [&](auto slot_tag, int k) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_tag)::value;
        TileRegsT<MASK, E::NQ>& tf = tf_[SLOT];
        if (SLOT == 0 && grp == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) plane_load<PMINOR>(ps, dp, rp, k, i);
        }
        if constexpr (IDXD) {
            if constexpr (SLOT == 0) idx_begin<FMINOR, 3>(ro, mr, of, k);
            else idx_next<FMINOR, 3>(ro, mr, of, k);
        }
#pragma unroll
        for (int q = 0; q < E::NQ; ++q) quad_load<FMINOR, MASK, 3, IDXD>(tf, of, cf, k, ke, q, ro);
    };
    if (active && n > 0) {
        first(std::integral_constant<int, 0>{}, kb);
        if constexpr (DEPTH > 1) {
            if (n > 1) first(std::integral_constant<int, DEPTH - 1>{}, kb + KTv);
        }
    }
    // A group's sequence is stage(0), mfma(0), stage(1), mfma(1), ... with a workgroup barrier behind every step; group 1 runs one
    // step behind group 0, so every group passes 2 n + 1 barriers: group 1 one before its sequence, group 0 one behind it, a group
    // without a tile all of them.  (One loop over the 2 n + 1 phases with the step chosen inside joins the two steps' registers at
    // every phase: hipcc then keeps a second set of accumulators and copies the tile registers behind a wait for their loads.)
    if (!active) {
        for (int p = 0; p <= 2 * n; ++p) __syncthreads();
        return;
    }
    if (grp == 1) __syncthreads();
    for (int t = 0; t < n; ++t) {
        const int k0 = kb + t * KTv;
        unsigned* const Ad = As[SHARE == 1 ? (t & 1) : grp];
        unsigned* const Bd = Bs[SHARE == 2 ? (t & 1) : grp];
        unsigned* const Fd = SHARE == 2 ? Ad : Bd;
        unsigned* const Pd = SHARE == 2 ? Bd : Ad;
        // tile t + DEPTH / t + 1 exist: their requests go out with tile t's store
        const bool more = t + DEPTH < n, morep = t + 1 < n;
        const int kld = k0 + DEPTH * KTv, kpl = k0 + KTv;
        auto go = [&](auto slot_tag) __attribute__((always_inline)) {
            if (more) stage(Fd, Pd, k0, kld, kpl, VecTag{}, VecTag{}, slot_tag);
            else if (morep) stage(Fd, Pd, k0, k0, kpl, ScalarTag{}, VecTag{}, slot_tag);
            else stage(Fd, Pd, k0, k0, k0, ScalarTag{}, ScalarTag{}, slot_tag);
        };
        if (DEPTH == 1 || !(t & 1)) go(std::integral_constant<int, 0>{});
        else go(std::integral_constant<int, DEPTH - 1>{});
        __syncthreads();
        mfma_ktile<AMINOR, BMINOR, 3>(acc, Ad, Bd, wm, wn, lane);
        // (the MFMAs touch registers only, and hipcc moves the barrier up to where the fragment reads end: the step would then run
        // beside the other group's matrix step instead of its staging step.  The fence keeps the barrier behind the step.)
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    if (grp == 0) __syncthreads();
    gemm_epilogue(g, acc, m0, n0, wm, wn, lane, arm);
}

// fc11 forward + bias + reconstruction loss + dZ11.  The product is computed TRANSPOSED, z^T = W11 d10^T: MFMA rows are
// genes and columns are cells, so a lane's four consecutive accumulator registers are four consecutive genes of one
// cell -- 16 contiguous bytes of x, dZ11 and x_rec.  grid (cell tiles, gene splits NS, A): a block keeps its 128 cells'
// d10 (both K tiles, bf16) in LDS and walks the 128-gene tiles of its gene range; the next W11 tile is requested from
// memory before the epilogue of the current one.  K = fc_dim <= 128.
__global__ __launch_bounds__(256, 2) void k_bf16_fc11(const GemmArgs g_in) {
    const GemmArgs g = g_in;
    __shared__ __attribute__((aligned(16))) unsigned Ws[2][BT * LDB];   // W11 tile: [gene][k], two K tiles
    __shared__ __attribute__((aligned(16))) unsigned Ds[2][BT * LDB];   // d10 tile: [cell][k], two K tiles
    __shared__ float red[8];
    const int arm = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int l31 = lane & 31, hh = lane >> 5;
    Operand od_h = g.a, ow_h = g.b;                   // a: d10 [B][H]; b: W11 [D][H]
    od_h.ptr += (int64_t)arm * g.a_arm;
    ow_h.ptr += (int64_t)arm * g.b_arm;
    const OperandDev od = make_operand_dev<false>(od_h), ow = make_operand_dev<false>(ow_h);
    const int c0 = blockIdx.x * BT;                    // cells of this block
    const int tiles = cdiv(g.N, BT);                   // gene tiles
    const int t0 = (int)(((int64_t)blockIdx.y * tiles) / g.KS), t1 = (int)(((int64_t)(blockIdx.y + 1) * tiles) / g.KS);
    const int K = g.K;
    const float* xa = g.fo.x + (int64_t)arm * g.fo_x_arm;
    float* dza = g.fo.dz + (int64_t)arm * g.fo_arm;
    float* xra = g.fo.x_rec ? g.fo.x_rec + (int64_t)arm * g.fo_arm : nullptr;
    const float* bias = g.fo.bias + (int64_t)arm * g.bias_arm;
    const int B = g.fo.B, D = g.fo.D;
    {
        TileRegsT<false> t0r, t1r;
        tile_load<false, false>(t0r, od, c0, 0, K);
        tile_load<false, false>(t1r, od, c0, KT, K);
        tile_store<false, false>(Ds[0], t0r, od, c0, 0, K);
        tile_store<false, false>(Ds[1], t1r, od, c0, KT, K);
    }
    TileRegsT<false> w0, w1;
    if (t0 < t1) {
        tile_load<false, false>(w0, ow, t0 * BT, 0, K);
        tile_load<false, false>(w1, ow, t0 * BT, KT, K);
    }
    float se = 0.f;
    int mism = 0;
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * BT;
        tile_store<false, false>(Ws[0], w0, ow, j0, 0, K);
        tile_store<false, false>(Ws[1], w1, ow, j0, KT, K);
        __syncthreads();
        if (t + 1 < t1) {
            tile_load<false, false>(w0, ow, j0 + BT, 0, K);
            tile_load<false, false>(w1, ow, j0 + BT, KT, K);
        }
        // the epilogue walks the four 32 x 32 pieces (i, j) of this wave's tile with the NEXT piece's x and bias in flight:
        // piece 0 is requested before the MFMAs, piece p + 1 before piece p is processed (140 -> 131 us; swapping
        // registers between the half-waves for 32-byte runs per lane, v_permlane32_swap, measured slower: 146 us)
        float4 xin[2][4], b4[2][4];
        auto request = [&](int pc, float4 (&X)[4], float4 (&Bq)[4]) __attribute__((always_inline)) {
            const int i = pc >> 1, j = pc & 1;
            const int cell = c0 + 64 * wn + 32 * j + l31;
            const int64_t rowoff = (int64_t)min(cell, B - 1) * D;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gene = j0 + 64 * wm + 32 * i + 8 * q + 4 * hh;
                const int gc = min(gene, D - 4);                      // D % 4 == 0
                X[q] = *reinterpret_cast<const float4*>(xa + rowoff + gc);
                Bq[q] = *reinterpret_cast<const float4*>(bias + gc);
            }
        };
        request(0, xin[0], b4[0]);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
        mfma_ktile<false, false>(acc, Ws[0], Ds[0], wm, wn, lane);
        if (K > KT) mfma_ktile<false, false>(acc, Ws[1], Ds[1], wm, wn, lane);
        // acc[i][j][4 q + e]: gene j0 + 64 wm + 32 i + 8 q + 4 hh + e, cell c0 + 64 wn + 32 j + (lane & 31)
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
            const int i = pc >> 1, j = pc & 1;
            if (pc + 1 < 4) request(pc + 1, xin[(pc + 1) & 1], b4[(pc + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const int cell = c0 + 64 * wn + 32 * j + l31;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gene = j0 + 64 * wm + 32 * i + 8 * q + 4 * hh;
                const bool ok = cell < B && gene < D;
                const float4 xq = xin[pc & 1][q], bq = b4[pc & 1][q];
                const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
                const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
                float xr[4], dz[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xr[e] = fmaxf(acc[i][j][4 * q + e] + bv[e], 0.f);
                    const float er = xr[e] - xv[e];
                    dz[e] = xr[e] > 0.f ? g.fo.coef * er : 0.f;
                    se += ok ? er * er : 0.f;
                    mism += (ok && ((xr[e] > 0.1f) != (xv[e] > 0.1f))) ? 1 : 0;
                }
                if (ok) {
                    *reinterpret_cast<float4*>(dza + (int64_t)cell * D + gene) = make_float4(dz[0], dz[1], dz[2], dz[3]);
                    if (xra) *reinterpret_cast<float4*>(xra + (int64_t)cell * D + gene) = make_float4(xr[0], xr[1], xr[2], xr[3]);
                }
            }
            // piece fence: keeps the requests one piece ahead (all four up front cost 128 registers and spill)
            asm volatile("" : "+v"(mism), "+v"(se));
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    se = wave_sum(se);
    const float mf = wave_sum((float)mism);
    if (lane == 0) { red[wv * 2] = se; red[wv * 2 + 1] = mf; }
    __syncthreads();
    if (tid == 0) {
        float* p = g.fo.part + ((int64_t)arm * g.n11 + (int64_t)blockIdx.x * g.KS + blockIdx.y) * 2;
        p[0] = red[0] + red[2] + red[4] + red[6];
        p[1] = red[1] + red[3] + red[5] + red[7];
    }
}

// fc11 forward + bias + reconstruction loss + dZ11 + d(d10), train step: k_bf16_fc11 with the second GEMM folded in, so
// dZ11 is not read back from HBM (200 MB per step at the benchmark shape) and one launch disappears.  Wave w of the four
// owns cells [32 w, 32 w + 32) of the block's 128 and ALL 128 genes of the current gene tile (four 32 x 32 accumulators,
// computed and consumed two at a time).  The dZ11 piece a wave has just formed IS the next MFMA's operand: the
// accumulator layout has the cell on the lane and four genes per register group, which is the A operand of
// d(d10)[cell][h] += sum_gene dZ11[cell][gene] W11[gene][h] once the sixteen genes of a K step are taken in the order
// the registers hold them (lower half-wave: genes 0-3, 8-11; upper: 4-7, 12-15 of the block of 16) -- no LDS round trip,
// no lane movement.  The B operand uses the same order: W11[gene][h] for four consecutive genes and one h per lane comes
// out of the [gene][h] image that is in LDS anyway through the transposing read (two ds_read_b64_tr_b16).  The d(d10)
// accumulators (32 cells x 128 h per wave) live across the whole gene range and are written once, to the gene-split slab.
// S16 (bf16 storage): x is read from its bf16 copy (g.fo.x addresses 2-byte elements; the loss and dZ11 then see the rounded
// x) and dZ11 is WRITTEN as bf16 (g.fo.dz likewise) -- exactly the values the d(d10) product here and the dW11 GEMM take
// anyway, so only the loss's view of x changes; the kernel moves 2 x 2 + 2 bytes per cell and gene instead of 2 x 4 + 4.
// W16: W11 is read from slice 0 of its planes ([D -> rup 128][128] bf16, launch_x3_planes) in sixteen-byte pieces of eight elements
// that go to the LDS image as they are, instead of fp32 rounded by every block (half the bytes from L2, no conversion; the
// timing ablation prices the fp32 tiles at 13 of the kernel's 84 us: profiles/r04_bf16_fc11g_ablation.txt; 84 -> 75 us.  Requesting
// x one half tile ahead in the registers this frees was measured too: 75.1 against 74.5 us, not kept)
static_assert(KT == 64, "W16: a row of W11's planes (128 bf16) is exactly the two K tiles in LDS");
template <bool S16, bool W16 = false>
__global__ __launch_bounds__(256, 2) void k_bf16_fc11g(const GemmArgs g_in) {
    const GemmArgs g = g_in;
    __shared__ __attribute__((aligned(16))) unsigned Ws[2][BT * LDB];   // W11 tile: [gene][k = h], two K tiles
    __shared__ __attribute__((aligned(16))) unsigned Ds[2][BT * LDB];   // d10 tile: [cell][k = h], two K tiles
    __shared__ __attribute__((aligned(16))) float bias_s[BT];
    __shared__ float red[8];
    const int arm = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    Operand od_h = g.a, ow_h = g.b;                   // a: d10 [B][H]; b: W11 [D][H]
    od_h.ptr += (int64_t)arm * g.a_arm;
    ow_h.ptr += (int64_t)arm * g.b_arm;
    const OperandDev od = make_operand_dev<false>(od_h), ow = make_operand_dev<false>(ow_h);
    const int c0 = blockIdx.x * BT;
    const int tiles = cdiv(g.N, BT);
    const int t0 = (int)(((int64_t)blockIdx.y * tiles) / g.KS), t1 = (int)(((int64_t)(blockIdx.y + 1) * tiles) / g.KS);
    const int K = g.K;
    const int ksteps1 = K > KT ? cdiv(K - KT, 16) : 0;      // MFMA steps of the second K tile that hold any k < K
    const float* xa = g.fo.x + (int64_t)arm * g.fo_x_arm;
    float* dza = g.fo.dz + (int64_t)arm * g.fo_arm;
    const float* bias = g.fo.bias + (int64_t)arm * g.bias_arm;
    const int B = g.fo.B, D = g.fo.D;
    {
        TileRegsT<false> t0r, t1r;
        tile_load<false, false>(t0r, od, c0, 0, K);
        tile_load<false, false>(t1r, od, c0, KT, K);
        tile_store<false, false>(Ds[0], t0r, od, c0, 0, K);
        tile_store<false, false>(Ds[1], t1r, od, c0, KT, K);
    }
    TileRegsT<false> w0, w1;
    OctRegs wo0, wo1;
    const unsigned no_map[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto w_request = [&](int j) __attribute__((always_inline)) {
        if constexpr (W16) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                oct_load<false, false>(wo0, ow, j, 0, 2 * KT, p, no_map);
                oct_load<false, false>(wo1, ow, j, KT, 2 * KT, p, no_map);
            }
        } else {
            tile_load<false, false>(w0, ow, j, 0, K);
            tile_load<false, false>(w1, ow, j, KT, K);
        }
    };
    auto w_store = [&](int j) __attribute__((always_inline)) {
        if constexpr (W16) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                oct_store<false>(Ws[0], wo0, ow, j, 0, 2 * KT, p);
                oct_store<false>(Ws[1], wo1, ow, j, KT, 2 * KT, p);
            }
        } else {
            tile_store<false, false>(Ws[0], w0, ow, j, 0, K);
            tile_store<false, false>(Ws[1], w1, ow, j, KT, K);
        }
    };
    float bnext = 0.f;
    if (t0 < t1) {
        w_request(t0 * BT);
        if (tid < BT) bnext = bias[min(t0 * BT + tid, D - 1)];
    }
    f32x16 gd[4] = {zero16(), zero16(), zero16(), zero16()};   // d(d10)[cell = 32 wv + row][h = 32 nt + (lane & 31)]
    float se = 0.f;
    int mism = 0;
    const int cell = c0 + 32 * wv + l31;
    const int64_t rowoff = g.fo.xmap ? (int64_t)g.fo.xmap[min(cell, B - 1)] : (int64_t)min(cell, B - 1) * D;   // (row map: the batch is rows of the resident matrix)
    const unsigned short* Wk16[2] = {reinterpret_cast<const unsigned short*>(Ws[0]), reinterpret_cast<const unsigned short*>(Ws[1])};
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
    // transposing-read address of this lane inside a (4 genes x 16 h) block: row (lane & 15) >> 2, columns 4 (lane & 3) ..
    const int tr_off = ((lane & 15) >> 2) * (2 * LDB) + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * BT;
        w_store(j0);
        if (tid < BT) bias_s[tid] = bnext;
        __syncthreads();
        if (t + 1 < t1) {
            w_request(j0 + BT);
            if (tid < BT) bnext = bias[min(j0 + BT + tid, D - 1)];
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            // x of the two gene sub-tiles of this half (requested before the MFMAs that produce their z)
            // S16: a lane's four genes of a group are 8 bytes; the two half-waves of a cell (lanes l, l + 32: genes 8 q + 0 .. 3
            // and 8 q + 4 .. 7) instead request SIXTEEN bytes each -- the lower lane the whole group q = 2 qp, the upper one the
            // whole group 2 qp + 1 -- and trade halves with v_permlane32_swap where the values are used (and the other way
            // round for the dZ11 store): half the vector-memory instructions, and every store covers an aligned 16 bytes
            // (as 8-byte stores dZ11 cost 1.5 x its bytes in partially written lines, PMC)
            float4 xin[2][4];
            u32x4v xraw[2][2];
#pragma unroll
            for (int gl = 0; gl < 2; ++gl) {
                if constexpr (S16) {
#pragma unroll
                    for (int qp = 0; qp < 2; ++qp) {
                        const int gene = j0 + 32 * (2 * half + gl) + 8 * (2 * qp + hh);                   // D % 8 == 0
                        xraw[gl][qp] = *reinterpret_cast<const u32x4v*>(reinterpret_cast<const unsigned short*>(xa) + rowoff + min(gene, D - 8));
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int gene = j0 + 32 * (2 * half + gl) + 8 * q + 4 * hh;
                        xin[gl][q] = *reinterpret_cast<const float4*>(xa + rowoff + min(gene, D - 4));      // D % 4 == 0
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc[2] = {zero16(), zero16()};       // z^T[gene sub-tile 2 half + gl][this wave's 32 cells]
#pragma unroll
            for (int s = 0; s < KT / 16; ++s) {
                const bf16x8 b = frag8<false>(Ds[0], 32 * wv, s, lane);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag8<false>(Ws[0], 32 * (2 * half), s, lane), b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag8<false>(Ws[0], 32 * (2 * half + 1), s, lane), b, acc[1], 0, 0, 0);
            }
            for (int s = 0; s < ksteps1; ++s) {
                const bf16x8 b = frag8<false>(Ds[1], 32 * wv, s, lane);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag8<false>(Ws[1], 32 * (2 * half), s, lane), b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag8<false>(Ws[1], 32 * (2 * half + 1), s, lane), b, acc[1], 0, 0, 0);
            }
#pragma unroll
            for (int gl = 0; gl < 2; ++gl) {
                const int gi = 2 * half + gl;
                // acc[gl][4 q + e]: gene j0 + 32 gi + 8 q + 4 hh + e of cell `cell`
                float dzr[16];
                if constexpr (S16) {
                    // lanes l / l + 32 hold (group 2 qp | group 2 qp + 1) whole: swap(lo, hi) hands every lane its own
                    // four genes of both groups
#pragma unroll
                    for (int qp = 0; qp < 2; ++qp) {
                        const auto s0 = __builtin_amdgcn_permlane32_swap(xraw[gl][qp][0], xraw[gl][qp][2], false, false);
                        const auto s1 = __builtin_amdgcn_permlane32_swap(xraw[gl][qp][1], xraw[gl][qp][3], false, false);
                        xin[gl][2 * qp] = make_float4(__uint_as_float(s0[0] << 16), __uint_as_float(s0[0] & 0xFFFF0000u),
                                                      __uint_as_float(s1[0] << 16), __uint_as_float(s1[0] & 0xFFFF0000u));
                        xin[gl][2 * qp + 1] = make_float4(__uint_as_float(s0[1] << 16), __uint_as_float(s0[1] & 0xFFFF0000u),
                                                          __uint_as_float(s1[1] << 16), __uint_as_float(s1[1] & 0xFFFF0000u));
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int gene = j0 + 32 * gi + 8 * q + 4 * hh;
                    const bool ok = cell < B && gene < D;
                    const float4 xq = xin[gl][q];
                    const float4 bq = *reinterpret_cast<const float4*>(&bias_s[32 * gi + 8 * q + 4 * hh]);
                    const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
                    const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float xr = fmaxf(acc[gl][4 * q + e] + bv[e], 0.f);
                        const float er = xr - xv[e];
                        dzr[4 * q + e] = (ok && xr > 0.f) ? g.fo.coef * er : 0.f;
                        se += ok ? er * er : 0.f;
                        mism += (ok && ((xr > 0.1f) != (xv[e] > 0.1f))) ? 1 : 0;
                    }
                    if constexpr (!S16) {
                        if (ok) *reinterpret_cast<float4*>(dza + (int64_t)cell * D + gene) =
                            make_float4(dzr[4 * q], dzr[4 * q + 1], dzr[4 * q + 2], dzr[4 * q + 3]);
                    }
                }
                if constexpr (S16) {
#pragma unroll
                    for (int qp = 0; qp < 2; ++qp) {
                        const int qe = 2 * qp, qo = 2 * qp + 1;
                        const auto s0 = __builtin_amdgcn_permlane32_swap(pack_bf16(dzr[4 * qe], dzr[4 * qe + 1]), pack_bf16(dzr[4 * qo], dzr[4 * qo + 1]), false, false);
                        const auto s1 = __builtin_amdgcn_permlane32_swap(pack_bf16(dzr[4 * qe + 2], dzr[4 * qe + 3]), pack_bf16(dzr[4 * qo + 2], dzr[4 * qo + 3]), false, false);
                        u32x4v w;
                        w[0] = s0[0]; w[1] = s1[0]; w[2] = s0[1]; w[3] = s1[1];
                        const int gene = j0 + 32 * gi + 8 * (2 * qp + hh);
                        if (cell < B && gene < D) *reinterpret_cast<u32x4v*>(reinterpret_cast<unsigned short*>(dza) + (int64_t)cell * D + gene) = w;
                    }
                }
                // d(d10) += dZ11 piece (registers) x W11 rows 32 gi .. + 31 (LDS): two K steps of sixteen genes
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    u32x4v au;
                    au[0] = pack_bf16(dzr[8 * c + 0], dzr[8 * c + 1]);
                    au[1] = pack_bf16(dzr[8 * c + 2], dzr[8 * c + 3]);
                    au[2] = pack_bf16(dzr[8 * c + 4], dzr[8 * c + 5]);
                    au[3] = pack_bf16(dzr[8 * c + 6], dzr[8 * c + 7]);
                    const bf16x8 afr = __builtin_bit_cast(bf16x8, au);
                    const int grow = 32 * gi + 16 * c + 4 * hh;            // first of this lane's two gene groups (second: + 8)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const unsigned short* a = Wk16[nt >> 1] + grow * (2 * LDB) + 32 * (nt & 1) + tr_off;
                        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)a);
                        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(a + 8 * (2 * LDB)));
                        typedef short s16x8 __attribute__((ext_vector_type(8)));
                        s16x8 r;
                        r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
                        r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
                        gd[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr, __builtin_bit_cast(bf16x8, r), gd[nt], 0, 0, 0);
                    }
                }
                asm volatile("" : "+v"(mism), "+v"(se));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();
    }
    // ---- d(d10) partial of this gene range: slab [NS][A][B][H]; gd[nt][r]: cell row acc_row(r), h = 32 nt + (lane & 31)
    {
        const int H = g.K;
        float* out = g.so.out + (int64_t)blockIdx.y * g.so.ks_stride + (int64_t)arm * g.so.arm_stride;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int h = 32 * nt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = c0 + 32 * wv + acc_row(r, lane);
                if (row < B && h < H) out[(int64_t)row * H + h] = gd[nt][r];
            }
        }
    }
    se = wave_sum(se);
    const float mf = wave_sum((float)mism);
    if (lane == 0) { red[wv * 2] = se; red[wv * 2 + 1] = mf; }
    __syncthreads();
    if (tid == 0) {
        float* p = g.fo.part + ((int64_t)arm * g.n11 + (int64_t)blockIdx.x * g.KS + blockIdx.y) * 2;
        p[0] = red[0] + red[2] + red[4] + red[6];
        p[1] = red[1] + red[3] + red[5] + red[7];
    }
}

// fc11 forward + bias + reconstruction loss + dZ11 + d(d10) of the fp32x3 configuration (the train step's dominant kernel).
// Same mathematics and data flow as k_bf16_fc11g -- z^T = W11 d10^T on the matrix pipe with the cell on the lane, the
// dZ11 piece in the accumulator IS the next product's operand -- with every operand as three bf16 slices and six slice
// products per product:
//   * [W11 | b11] and [d10 | 1] arrive as slice planes (k_presplit, once per step): the bias rides as k = fc_dim, so the
//     accumulator already holds z + b and the epilogue loads no bias;
//   * ONE WAVE PER SIMD (256 threads = 4 waves x 32 cells, up to 512 VGPRs each).  Two waves per SIMD at 256 registers
//     were measured first: a wave's VALU instructions hardly issue while its partner runs MFMAs (epilogue 1 860 cycles
//     alone, 3 600 - 4 700 beside the partner), the two waves ran in the sum of their times, and 256 registers left the
//     compiler no room to request LDS fragments ahead of the MFMAs that consume them.  With 512 registers the wave
//     overlaps its own work instead: the z product of piece p + 1 (42 MFMAs, fragments requested one K step ahead) is
//     issued through the epilogue of piece p (about six VALU instructions fit behind every MFMA);
//   * a wave keeps its cells' d10 slices in registers for the whole kernel (7 K steps x 3 slices x 4 VGPRs);
//   * LDS holds only W11 tiles (64 genes x 128 k x 3 slices, XOR-swizzled, 48 KB), three of them, filled by LDS-DMA
//     (global_load_lds_dwordx4: no registers, no VALU) two tiles ahead; a tile serves the z product as the A operand
//     (ds_read_b128) and the d(d10) product as the B operand through transposing reads (ds_read_b64_tr_b16);
//   * dZ11 is split into its slices in registers between the two products (eleven VALU instructions per pair);
//   * cells and genes that do not exist have z = 0 (zero rows of the planes) and read x = 0 (buffer range): no masks.
// grid (ceil(B / 128), gene splits NS, A); fc_dim + 1 <= 112.
// W11 tile image in LDS: [gene][k], 128 bf16 = 16 sixteen-byte blocks per row, NO padding; block c of row r sits at block
// c ^ fw_swz(r).  The image is read two ways -- row per lane (ds_read_b128: 16 lanes x 16 B must hit 16 different
// 4-bank groups) and transposed (ds_read_b64_tr_b16: per LDS cycle 2 x 16 lanes = 4 rows x 2 blocks x 2 column groups) --
// and no row pitch serves both (60 dwords: transposing reads 2-way conflicts, 19 % of the kernel's busy cycles in the PMC
// pass; 80: row reads 4-way).  The XOR below makes both conflict-free: rows r .. r + 3 differ in bits 2-3 of the block,
// rows r, r + 4, r + 8, r + 12 in bits 0-1.
constexpr int FW_ROW = 64;                     // dwords per W11 image row
constexpr int FW_PLANE = 64 * FW_ROW;          // dwords per slice image of a 64-gene tile
constexpr int FW_TILE = 3 * FW_PLANE;
__device__ __forceinline__ int fw_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__global__ __launch_bounds__(256, 1) void k_x3_fc11g(const GemmArgs g_in) {
    const GemmArgs g = g_in;
    __shared__ __attribute__((aligned(16))) unsigned Wl[3 * FW_TILE];        // three tiles
    __shared__ float red[8];
    const int arm = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const unsigned short* Wp = g.b.pl + (int64_t)arm * g.b.pl_arm;      // [3][Dr][128]
    const unsigned short* Dp = g.a.pl + (int64_t)arm * g.a.pl_arm;      // [3][Br][128]
    const int64_t wplane = g.b.pl_plane, dplane = g.a.pl_plane;
    const int B = g.fo.B, D = g.fo.D, H = g.K;
    const int c0 = blockIdx.x * 128;
    const int tiles = cdiv(D, 64);
    const int t0 = (int)(((int64_t)blockIdx.y * tiles) / g.KS), t1 = (int)(((int64_t)(blockIdx.y + 1) * tiles) / g.KS);
    const int cell = c0 + 32 * wv + l31;
    const float* xa = g.fo.x + (int64_t)arm * g.fo_x_arm;
    float* dza = g.fo.dz + (int64_t)arm * g.fo_arm;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xa), 0, (int)((g.fo.xmap ? g.fo.x_nrec : (int64_t)B * D) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(dza, 0, (int)((int64_t)B * D * 4), 0x00020000);
    // this lane's cell: its row of x (through the row map when the batch is not materialised) and of dZ11
    const int rowoff = g.fo.xmap ? (int)g.fo.xmap[min(cell, B - 1)] : min(cell, B - 1) * D;          // B * D < 2^30 (fast-path condition)
    const bool cell_ok = cell < B;
    int dzoff = min(cell, B - 1) * D * 4;          // byte offset of the lane's row of dZ11 (a register of its own: with the product
    asm volatile("" : "+v"(dzoff));                // inside the store's select hipcc branched around it, and a branch ends a region)
    int dlim = cell_ok ? D : 0;                    // genes this lane may touch (a per-lane bound instead of `cell_ok && gene < D`:
    asm volatile("" : "+v"(dlim));                 // a uniform-looking `cell_ok` became an exec-mask branch around the select)

    // LDS-DMA of W11 tile t into buffer (t - t0) % 3: 3 slices x 64 rows x 16 sixteen-byte blocks = 48 wave instructions of
    // 1 KB, twelve per wave; LDS slot (row, block b) takes the plane's block b ^ fw_swz(row) (blocks 14, 15: the planes'
    // zero padding).
    // Addressing is split into what depends on the lane (once, one VGPR: the byte offset of the lane's block inside the
    // first rows of a tile's plane; the swizzle term does not depend on j because rows advance by 16) and what is uniform
    // (per instruction: a 64-bit scalar base and the LDS address for M0, a few scalar adds).  Written with a pointer into
    // Wl and a per-lane source pointer, hipcc converted the generic LDS pointer to a local one (null check included) and
    // moved both halves through v_readfirstlane for every one of the twelve instructions: ~130 of the loop's ~1060
    // non-matrix instructions, in a kernel that is bound by instruction issue.
    const int wv_s = __builtin_amdgcn_readfirstlane(wv);
    const unsigned wl_base = (unsigned)(size_t)(__attribute__((address_space(3))) void*)(&Wl[0]);
    const int lrow = 4 * wv + (lane >> 4);                                  // the lane's row inside a 16-row group
    const unsigned dma_voff = 2u * ((unsigned)lrow * 128u + 8u * (unsigned)((lane & 15) ^ fw_swz(lrow)));
    auto dma = [&](int t) __attribute__((always_inline)) {
        const int buf = (t - t0) % 3;
        const unsigned lds0 = wl_base + 4u * (unsigned)(buf * FW_TILE) + 1024u * (unsigned)wv_s;
        const unsigned short* src0 = Wp + (int64_t)t * (64 * 128);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            // instruction j of this wave: slice j >> 2, rows 16 (j & 3) + 4 wv .. + 3 of the tile (one 1 KB LDS chunk)
            const unsigned short* src = src0 + (int64_t)(j >> 2) * wplane + (j & 3) * (16 * 128);
            const unsigned lds_addr = lds0 + 4u * (unsigned)((j >> 2) * FW_PLANE) + 4096u * (unsigned)(j & 3);
            // (inline assembly, not __builtin_amdgcn_global_load_lds: hipcc's wait-count pass treats the builtin as a store to
            // "some" LDS and puts s_waitcnt vmcnt(0) in front of the next LDS read -- which, with the x prefetch just issued,
            // stalled every tile for a full memory round trip.  The waits for the DMA are the counted ones in the loop.)
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         :: "s"(lds_addr), "v"(dma_voff), "s"(src) : "memory");
        }
    };
    if (t0 < t1) dma(t0);
    if (t0 + 1 < t1) dma(t0 + 1);
    // this wave's d10 slices: lane = cell, K step s holds k = 16 s + 8 hh .. + 7
    bf16x8 dfr[7][3];
    {
        const int cr = min(cell, (int)(dplane / 128) - 1);
#pragma unroll
        for (int s = 0; s < 7; ++s)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                dfr[s][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(Dp + (int64_t)pl * dplane + (int64_t)cr * 128 + 16 * s + 8 * hh));
    }
    f32x16 gd[4] = {zero16(), zero16(), zero16(), zero16()};   // d(d10)[cell = 32 wv + row][h = 32 nt + (lane & 31)]
    float seq[4] = {0.f, 0.f, 0.f, 0.f};
    int mism = 0;                       // wave-uniform: mismatches of the whole wave
    typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    // transposing read: this lane supplies the address of row q = (lane & 15) >> 2 of a (4 genes x 16 h) block, columns
    // 4 (lane & 3) .. + 3 of the 16 that start at 16 ((lane >> 4) & 1): sixteen-byte block 2 ((lane >> 4) & 1) + (lane & 3) / 2
    // of the h tile, its half (lane & 1)
    const int tr_q = (lane & 15) >> 2, tr_blk = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1), tr_half = 4 * (lane & 1);
    const int npieces = 2 * (t1 - t0);
    // piece p: genes [64 t0 + 32 p, + 32), rows 32 (p & 1) of tile t0 + p / 2 in LDS buffer (p / 2) % 3
    auto w_rows = [&](int p) __attribute__((always_inline)) { return Wl + ((p >> 1) % 3) * FW_TILE + 32 * (p & 1) * FW_ROW; };
    const int a_swz = fw_swz(l31);      // (a piece starts at row 0 or 32 of the tile: the row's low four bits are the lane's)
    auto a_frag = [&](const unsigned* Wr, int s, int pl) __attribute__((always_inline)) {
        return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(Wr + pl * FW_PLANE + l31 * FW_ROW + 4 * ((2 * s + hh) ^ a_swz)));
    };
    auto request_x = [&](float4 (&X)[4], int j0g, int q) __attribute__((always_inline)) {   // x of gene group q of the piece at j0g
        const int gene = j0g + 8 * q + 4 * hh;                      // D % 4 == 0: a float4 exists entirely or not at all
        int off = gene < dlim ? (rowoff + gene) * 4 : -16;
        asm("" : "+v"(off));       // (a plain select: hipcc otherwise branches around two copies of the load, and a branch
                                   // ends the region in which MFMAs and VALU instructions can be interleaved)
        X[q] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
    };
    // six slice products of one K step
    // (one accumulation chain: dependent MFMAs of this shape issue back to back, tools/micro/x3_issue_bench.hip)
    auto mfma6 = [&](f32x16& acc, const bf16x8 (&a)[3], int s) __attribute__((always_inline)) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], dfr[s][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], dfr[s][2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], dfr[s][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], dfr[s][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], dfr[s][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], dfr[s][0], acc, 0, 0, 0);
    };
    // ------------------------------------------------------------------------------------------------------------
    // One piece = stage 1 (the z product of the NEXT piece, 42 MFMAs in seven regions of one K step, with this piece's
    // epilogue cut into eight chunks of VALU work behind them) + stage 2 (this piece's d(d10) product, 48 MFMAs in four
    // regions).  Every LDS fragment is requested TWO regions before the MFMAs that consume it (a ds_read costs 64+ cycles
    // when it is waited for at once -- tools/micro/x3_issue_bench.hip -- and hipcc sinks reads towards their uses, so the
    // regions are fenced with sched_barrier and the requests placed by hand); the rings of fragments carry over from
    // piece to piece.  Accumulators live in the accumulator half of the register file (this file is compiled without
    // -amdgpu-mfma-vgpr-form), which leaves the architectural VGPRs to the fragments in flight.
    // ------------------------------------------------------------------------------------------------------------
    bf16x8 an[3][3];          // A fragments (W11 slices) of the z product: ring over K steps
    bf16x8 wq[2][2][3];       // transposed W11 fragments of the d(d10) product: ring over regions; [h tile of the pair][slice]
    auto z_frags = [&](const unsigned* Wr, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) an[s % 3][pl] = a_frag(Wr, s, pl);
    };
    auto d_frags = [&](const unsigned short* Wt16, int r) __attribute__((always_inline)) {   // region r: K step r >> 1, h tiles 2 (r & 1) ..
        const int row0 = 16 * (r >> 1) + 4 * hh + tr_q;     // this lane's row of the first gene group (second: + 8)
        const int sw0 = fw_swz(row0), sw1 = fw_swz(row0 + 8);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const int blk = 4 * (2 * (r & 1) + j) + tr_blk;     // sixteen-byte block of the row (h tile 2 (r & 1) + j)
                const unsigned short* base = Wt16 + pl * (2 * FW_PLANE) + tr_half;
                const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + row0 * (2 * FW_ROW) + 8 * (blk ^ sw0)));
                const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + (row0 + 8) * (2 * FW_ROW) + 8 * (blk ^ sw1)));
                s16x8 rr;
                rr[0] = v0[0]; rr[1] = v0[1]; rr[2] = v0[2]; rr[3] = v0[3];
                rr[4] = v1[0]; rr[5] = v1[1]; rr[6] = v1[2]; rr[7] = v1[3];
                wq[r & 1][j][pl] = __builtin_bit_cast(bf16x8, rr);
            }
    };
    float4 xa_[4], xb_[4];
    f32x16 acc_a = zero16();
    // The d10 slices are complete HERE, on every path into the main loop (they live in the accumulator half of the register
    // file from now on: only MFMAs read them).  With this wait inside the `if` below, the path around it -- a block without
    // tiles, which never runs the loop, but hipcc cannot know -- carried "d10 still in flight" to the loop header, and the
    // wait-count pass put vmcnt(24) / (22) / (7) in front of the first MFMAs of EVERY piece: "all but the seven youngest
    // vector-memory operations have completed" right behind the four x requests, i.e. a wait for the previous piece's stores
    // and for the W11 tile requested half a tile earlier -- 50 us of the kernel's 155 (no-load and no-store ablations).
    __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
#pragma unroll
    for (int s7 = 0; s7 < 7; ++s7)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) asm volatile("" : "+a"(dfr[s7][pl]));
    if (npieces > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) request_x(xa_, t0 * 64, q);
        __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0): both first tiles and x
        // (hipcc's wait-count pass does not see that wait: without a use of the registers HERE it keeps "x may still be in
        // flight" alive around the loop's back edge)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(xa_[q].x), "+v"(xa_[q].y), "+v"(xa_[q].z), "+v"(xa_[q].w));
        __syncthreads();
        if (t0 + 2 < t1) dma(t0 + 2);
        // z of piece 0
        const unsigned* Wr = w_rows(0);
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            bf16x8 a[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) a[pl] = a_frag(Wr, s, pl);
            mfma6(acc_a, a, s);
        }
        const unsigned* W1 = w_rows(npieces > 1 ? 1 : 0);
        z_frags(W1, 0);
        z_frags(W1, 1);
    }
    // piece p: epilogue reads `acc` / `xin`, the z product of piece p + 1 goes to `accn`, its x to `xnx`
    // (ONE z accumulator: the piece copies its z out of the accumulator registers at its head -- the epilogue's VALU
    // instructions cannot read those anyway -- and the next piece's product goes into the same registers.  With two
    // accumulators swapped from piece to piece hipcc parked d(d10)'s first tile in VGPRs around every z product: 32 more
    // accumulator copies per tile.)
    auto piece = [&](int p, f32x16& accn, float4 (&xin)[4], float4 (&xnx)[4], int dma_tile) __attribute__((always_inline)) {
        const int j0g = t0 * 64 + 32 * p;
        const unsigned* Wn = w_rows(p + 1 < npieces ? p + 1 : p);
        const unsigned short* Wt16 = reinterpret_cast<const unsigned short*>(w_rows(p));
        f32x16 acc = accn;
        asm volatile("" : "+v"(acc));
        accn = zero16();
        unsigned au[2][3][4];          // dZ11 slices: K step c (sixteen genes in register order), slice, four dwords
        float dzq[4];
        // x of the next piece first: requested in front of this piece's stores, the wait for it (vector-memory instructions
        // retire in order) then does not include them
#pragma unroll
        for (int q = 0; q < 4; ++q) request_x(xnx, j0g + 32, q);
        // chunk 2 q: loss terms, dZ11 and its store for gene group q (acc[4 q + e] is gene j0g + 8 q + 4 hh + e of cell
        // `cell`); chunk 2 q + 1: its slices.  Eight VALU instructions per element; the mismatch count is kept on the scalar
        // unit (lane-mask population counts), outside the VALU's dependency chains.
        auto chunk = [&](int ch) __attribute__((always_inline)) {
            const int q = ch >> 1;
            if ((ch & 1) == 0) {
                const int gene = j0g + 8 * q + 4 * hh;
                const float xv[4] = {xin[q].x, xin[q].y, xin[q].z, xin[q].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a_ = acc[4 * q + e];
                    // max(z, 0) as ONE instruction: a signed-integer maximum of the bit pattern (fmaxf also canonicalises
                    // its input -- a second v_max_f32 per element)
                    const float xr = __int_as_float(max(__float_as_int(a_), 0));
                    const float er = xr - xv[e];
                    seq[q] = __builtin_fmaf(er, er, seq[q]);
                    const float d_ = g.fo.coef * er;
                    dzq[e] = a_ > 0.f ? d_ : 0.f;
                    mism += __builtin_popcountll(__builtin_amdgcn_ballot_w64(xr > 0.1f) ^ __builtin_amdgcn_ballot_w64(xv[e] > 0.1f));
                }
                // (always issued -- the counted wait at the end of a tile relies on it; what must not be written gets an offset
                // beyond the buffer's range, which the hardware drops)
                int soff = gene < dlim ? dzoff + gene * 4 : -16;
                asm("" : "+v"(soff));
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, make_float4(dzq[0], dzq[1], dzq[2], dzq[3])), rz, soff, 0, 0);
            } else {
                unsigned w0[3], w1[3];
                split3(dzq[0], dzq[1], w0);
                split3(dzq[2], dzq[3], w1);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) { au[q >> 1][pl][2 * (q & 1)] = w0[pl]; au[q >> 1][pl][2 * (q & 1) + 1] = w1[pl]; }
            }
        };
        // (this piece's x was requested a piece ago: one wait for all of it here, in front of the DMA's assembly -- see below)
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(xin[q].x), "+v"(xin[q].y), "+v"(xin[q].z), "+v"(xin[q].w));
        // ---- stage 1: seven regions of six MFMAs; chunks 0 .. 4 of the epilogue behind them (the other three go behind the
        // first MFMAs of stage 2, which has no other VALU work: 42 MFMAs + 5 chunks against 48 MFMAs + 3 chunks)
#pragma unroll
        for (int s = 0; s < 7; ++s) {
            __builtin_amdgcn_sched_barrier(0);
            if (s + 2 < 7) z_frags(Wn, s + 2);
            if (s == 5) d_frags(Wt16, 0);           // (the first region of stage 2: its slot of the ring is free)
            mfma6(accn, an[s % 3], s);
            if (s < 5) chunk(s);
        }
        asm volatile("" : "+s"(mism));
        // the DMA of a later tile goes here, behind the last use of this piece's x: hipcc does not count the assembly's
        // instructions, so a wait it places for a register loaded BEFORE them also waits for them
        if (dma_tile >= 0) dma(dma_tile);
        // ---- stage 2: d(d10) += dZ11 piece (registers) x W11 rows of piece p (LDS, transposed)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __builtin_amdgcn_sched_barrier(0);
            if (r + 1 < 4) d_frags(Wt16, r + 1);    // the other slot of the ring (region r - 1 is done with it)
            if (r >= 2) {
                // the first two K steps of the next piece's z product (piece p + 2: its tile has landed -- it is the tile of
                // piece p + 1 or the one the barrier at the end of the previous tile waited for)
                const unsigned* W2 = w_rows(p + 2 < npieces ? p + 2 : p);
                z_frags(W2, r - 2);
            }
            if (r == 0) { chunk(5); chunk(6); }       // (gene groups 2 and 3 feed K step 1 = regions 2 and 3)
            if (r == 1) chunk(7);
            const int c = r >> 1;
            bf16x8 af[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                u32x4v u;
                u[0] = au[c][pl][0]; u[1] = au[c][pl][1]; u[2] = au[c][pl][2]; u[3] = au[c][pl][3];
                af[pl] = __builtin_bit_cast(bf16x8, u);
            }
            // product-major: consecutive MFMAs go to the two h tiles of the region (independent accumulators)
            const int n0 = 2 * (r & 1);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[2], wq[r & 1][j][0], gd[n0 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], wq[r & 1][j][2], gd[n0 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], wq[r & 1][j][1], gd[n0 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[1], wq[r & 1][j][0], gd[n0 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], wq[r & 1][j][1], gd[n0 + j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) gd[n0 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[0], wq[r & 1][j][0], gd[n0 + j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int t = t0; t < t1; ++t) {
        const int p = 2 * (t - t0);
        // the first piece of tile t also requests tile t + 2 (into the buffer of tile t - 1, which every wave left at the
        // barrier below; tiles t0 .. t0 + 2 were requested by the prologue)
        piece(p, acc_a, xa_, xb_, (t > t0 && t + 2 < t1) ? t + 2 : -1);
        piece(p + 1, acc_a, xb_, xa_, -1);
        // ---- end of a tile (two pieces): tile t + 2 is needed next (the z product runs one piece ahead).  It was requested
        // in front of eight younger vector-memory instructions (the second piece's 4 loads + 4 stores); vector-memory
        // instructions retire in order, so "at most four outstanding" (those stores) guarantees this wave's share of it has
        // landed, and the barrier that of the others.  The barrier also lets tile t's buffer be overwritten.
        __builtin_amdgcn_s_waitcnt(0x0F74);                // vmcnt(4)
        __syncthreads();
    }
    // ---- d(d10) partial of this gene range: slab [NS][A][B][H]; gd[nt][r]: cell row acc_row(r), h = 32 nt + (lane & 31)
    {
        float* out = g.so.out + (int64_t)blockIdx.y * g.so.ks_stride + (int64_t)arm * g.so.arm_stride;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int h = 32 * nt + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = c0 + 32 * wv + acc_row(r, lane);
                if (row < B && h < H) out[(int64_t)row * H + h] = gd[nt][r];
            }
        }
    }
    const float se = wave_sum((seq[0] + seq[1]) + (seq[2] + seq[3]));
    if (lane == 0) { red[wv * 2] = se; red[wv * 2 + 1] = (float)mism; }
    __syncthreads();
    if (tid == 0) {
        float* pp = g.fo.part + ((int64_t)arm * g.n11 + (int64_t)blockIdx.x * g.KS + blockIdx.y) * 2;
        pp[0] = (red[0] + red[2]) + (red[4] + red[6]);
        pp[1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
    // the loss finalisation sums all n11 slots of an arm: the first block of the arm clears the ones no block writes
    // (instead of a memset launch in front of the kernel)
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = (int)gridDim.x * g.KS * 2 + tid; i < 2 * g.n11; i += 256) g.fo.part[(int64_t)arm * g.n11 * 2 + i] = 0.f;
}

// fc11 of a decode (mmvae_decode, mmvae_state_changes): x_rec = relu([d10 | 1] [W11 | b11]^T) and nothing else -- no x, no
// loss, no dZ11, no d(d10).  Both operands come as the slice planes the decoder already has: [W11 | b11] from
// launch_dec_planes, [d10 | 1] from the decoder chain (the bias rides as k = fc_dim, so the accumulator holds z + b).
// NP = 3 (fp32x3): six slice products per K step in k_x3_fc11g's order; NP = 1 (bf16): slice 0 of each plane, i.e. the
// operands -- the bias among them -- rounded to bf16.  NK K steps of 16 cover fc_dim + 1 (7: <= 112, 8: <= 128).
// A wave keeps the [d10 | 1] slices of its 32 cells in registers (MFMA B operand, cell on the lane) and walks the gene
// range of its block in pieces of 32 genes, the W11 rows of the next piece requested while the current one multiplies;
// a lane stores four consecutive genes of its cell per accumulator quarter.  grid (ceil(B / 128), gene splits, A).
struct Fc11OutArgs {
    const unsigned short* wpl; int64_t w_plane, w_arm;    // [A][3][rup(D, 128)][128]
    const unsigned short* dpl; int64_t d_plane, d_arm;    // [A][3][rup(B, 256)][128]
    float* out;                                          // [A][B][D]
    int B, D, KS;
};
template <int NP, int NK>
__global__ __launch_bounds__(256, 1) void k_fc11_out(const Fc11OutArgs g) {
    const int arm = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int B = g.B, D = g.D;
    const int cell = blockIdx.x * 128 + 32 * wv + l31;
    const unsigned short* Wp = g.wpl + (int64_t)arm * g.w_arm;
    const unsigned short* Dp = g.dpl + (int64_t)arm * g.d_arm;
    bf16x8 dfr[NK][NP];
    {
        const int cr = min(cell, (int)(g.d_plane / 128) - 1);
#pragma unroll
        for (int s = 0; s < NK; ++s)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
                dfr[s][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(Dp + (int64_t)pl * g.d_plane + (int64_t)cr * 128 + 16 * s + 8 * hh));
    }
    const int npc = cdiv(D, 32);
    const int p0 = (int)(((int64_t)blockIdx.y * npc) / g.KS), p1 = (int)(((int64_t)(blockIdx.y + 1) * npc) / g.KS);
    // W11 rows 32 p + (lane & 31) of piece p exist in the planes (rup(D, 128) rows, zero beyond D)
    auto load_w = [&](int p, bf16x8 (&a)[NK][NP]) __attribute__((always_inline)) {
        const unsigned short* r = Wp + (int64_t)(32 * p + l31) * 128 + 8 * hh;
#pragma unroll
        for (int s = 0; s < NK; ++s)
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
                a[s][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(r + (int64_t)pl * g.w_plane + 16 * s));
    };
    float* orow = g.out + ((int64_t)arm * B + min(cell, B - 1)) * D;
    const bool cell_ok = cell < B;
    bf16x8 wa[NK][NP], wb[NK][NP];
    auto piece = [&](int p, const bf16x8 (&a)[NK][NP]) __attribute__((always_inline)) {
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            if constexpr (NP == 3) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][2], dfr[s][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][0], dfr[s][2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][1], dfr[s][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][1], dfr[s][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][0], dfr[s][1], acc, 0, 0, 0);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][0], dfr[s][0], acc, 0, 0, 0);
        }
        // acc[4 q + e]: gene 32 p + 8 q + 4 hh + e of cell `cell`; D % 4 == 0, so a group of four exists entirely or not at all
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int gene = 32 * p + 8 * q + 4 * hh;
            if (cell_ok && gene < D)
                *reinterpret_cast<float4*>(orow + gene) = make_float4(relu_keep_nan(acc[4 * q]), relu_keep_nan(acc[4 * q + 1]),
                                                                      relu_keep_nan(acc[4 * q + 2]), relu_keep_nan(acc[4 * q + 3]));
        }
    };
    if (p0 < p1) load_w(p0, wa);
    for (int p = p0; p < p1; p += 2) {
        if (p + 1 < p1) load_w(p + 1, wb);
        piece(p, wa);
        if (p + 1 >= p1) break;
        if (p + 2 < p1) load_w(p + 2, wa);
        piece(p + 1, wb);
    }
}

// The small-layer weight / bias gradients (twelve products per arm, out[m][n] = sum_b P[b][m] Q'[b][n], m <= 128,
// n + 1 <= 128, K = batch) on the split engine: the ping-pong kernel with ONE PRODUCT PER GROUP -- the two groups of a block
// take products 2 b and 2 b + 1 of the (product, arm) list, each with its own operands (both batch-reduced, i.e. K-minor;
// Q optionally BatchNorm-normalised on load and extended by the ones column of the bias gradient, as k_gemm_tn does).
// grid (ceil(ndesc * A / 2), KS).  2.4 GFLOP in all: 57 us on the fp32 matrix instruction (pipe 28 % busy).
__global__ __launch_bounds__(512, 1) void k_x3_small(const TnDescs descs, int ndesc, int A, int B, int KS) {
    typedef Eng<3> E;
    constexpr int KTv = E::KT;
    __shared__ __attribute__((aligned(16))) unsigned As[2][3 * E::PLANE];
    __shared__ __attribute__((aligned(16))) unsigned Bs[2][3 * E::PLANE];
    // (the group index as a scalar, as in k_x3_gemm: the group's product, its operands and whether it exists are then uniform)
    const int grp = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    const int tid = threadIdx.x & 255, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
    const int unit = 2 * blockIdx.x + grp;
    const bool active = unit < ndesc * A;
    const int di = active ? unit % ndesc : 0, arm = active ? unit / ndesc : 0;
    const TnDesc& dr = descs.d[di];
    const TnDesc d = {dr.P, dr.p_arm_stride, dr.ldp, dr.Mv, dr.Q, dr.q_arm_stride, dr.ldq, dr.Nv, dr.q_ones, dr.q_xmask,
                      dr.q_mean, dr.q_rstd, dr.out, dr.out_arm_stride, dr.out_ks_stride, dr.ldo};
    Operand oa_h{d.P + (int64_t)arm * d.p_arm_stride, d.ldp, d.Mv, B, 1, nullptr, 0, -1, nullptr, 0, 0, 0};
    Operand ob_h{d.Q + (int64_t)arm * d.q_arm_stride, d.ldq, d.Nv, B, 1, nullptr, 0, d.q_ones ? d.Nv : -1, nullptr, 0, 0, 0};
    OperandDev oa = make_operand_dev<true>(oa_h), ob = make_operand_dev<true>(ob_h);
    const bool bn = d.q_mean != nullptr;
    {
        const int r4 = (tid & 31) * 4;
        float sb[4] = {0.f, 0.f, 0.f, 0.f}, ml[4] = {1.f, 1.f, 1.f, 1.f};
        if (bn) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (r4 + e < d.Nv) { sb[e] = d.q_mean[(int64_t)arm * d.Nv + r4 + e]; ml[e] = d.q_rstd[(int64_t)arm * d.Nv + r4 + e]; }
        }
        ob.bn_sub = make_float4(sb[0], sb[1], sb[2], sb[3]);
        ob.bn_mul = make_float4(ml[0], ml[1], ml[2], ml[3]);
    }
    const int nkt = cdiv(B, KTv);
    const int kb = (int)(((int64_t)blockIdx.y * nkt) / KS) * KTv;
    const int ke = min(B, (int)(((int64_t)(blockIdx.y + 1) * nkt) / KS) * KTv);
    const int n = ke > kb ? cdiv(ke - kb, KTv) : 0;
    f32x16 acc[2][2] = {{zero16(), zero16()}, {zero16(), zero16()}};
    TileRegsT<false, E::NQ> ta, tb;
    const PieceCtx ca = piece_ctx<true, 3>(oa, 0), cb = piece_ctx<true, 3>(ob, 0);
    unsigned* const Ad = As[grp];
    unsigned* const Bd = Bs[grp];
    auto stage = [&](int kst, int kld, auto load_tag) __attribute__((always_inline)) {
        constexpr bool LOAD = decltype(load_tag)::value;
#pragma unroll
        for (int i = 0; i < E::NQ; ++i) {
            quad_store<true, false, 3>(Ad, ta, oa, ca, kst, ke, i);
            if constexpr (LOAD) quad_load<true, false, 3>(ta, oa, ca, kld, ke, i);
            quad_store<true, false, 3, true>(Bd, tb, ob, cb, kst, ke, i);
            if constexpr (LOAD) quad_load<true, false, 3>(tb, ob, cb, kld, ke, i);
        }
    };
    if (active && n > 0) {
#pragma unroll
        for (int i = 0; i < E::NQ; ++i) {
            quad_load<true, false, 3>(ta, oa, ca, kb, ke, i);
            quad_load<true, false, 3>(tb, ob, cb, kb, ke, i);
        }
    }
    // (the sequence and its 2 n + 1 barriers as in k_x3_gemm; both groups have the same role here)
    if (!active) {
        for (int p = 0; p <= 2 * n; ++p) __syncthreads();
        return;
    }
    if (grp == 1) __syncthreads();
    for (int t = 0; t < n; ++t) {
        const int k0 = kb + t * KTv;
        if (k0 + KTv < ke) stage(k0, k0 + KTv, VecTag{});
        else stage(k0, k0, ScalarTag{});
        __syncthreads();
        mfma_ktile<true, true, 3>(acc, Ad, Bd, wm, wn, lane);
        __builtin_amdgcn_sched_barrier(0);      // (keeps the barrier behind the MFMAs: see k_x3_gemm)
        __syncthreads();
    }
    if (grp == 0) __syncthreads();
    tile_out(d.out + (int64_t)blockIdx.y * d.out_ks_stride + (int64_t)arm * d.out_arm_stride, d.ldo, d.Mv, d.Nv + d.q_ones, acc, 0, 0, wm, wn, lane);
}

// ---------------------------------------------------------------------------------------------------------------
// host launchers (same workspace layouts and split factors as the fp32 fast path)
// ---------------------------------------------------------------------------------------------------------------
static Operand kmajor(const float* p, int64_t ld, int rows, int K) {
    Operand o{};
    o.ptr = p; o.ld = ld; o.rows = rows; o.K = K; o.ones_row = -1;
    return o;
}
static Operand kminor(const float* p, int64_t ld, int rows, int K) { Operand o = kmajor(p, ld, rows, K); o.kminor = 1; return o; }

// Slice planes of the four small operands (fp32x3 engine).  They are written at fixed points of the step -- W1 and
// [W11 | b11] at the start of the forward pass (launch_x3_planes), [d10 | 1] by the decoder chain, dZ1 by k_bn_bwd_apply
// behind the encoder's backward chain (Plan) -- and read by the GEMM launchers below, which only fill in the
// operand's plane fields.
enum { PL_W1 = 0, PL_W11 = 1, PL_D10 = 2, PL_DZ1 = 3 };
struct PlaneGeom { int R, C, Rp, Cp, ones_col; int64_t ws_off; };
static PlaneGeom plane_geom(const Ctx& c, int kind) {
    const mmvae_dims& d = c.d;
    switch (kind) {
        case PL_W1:  return PlaneGeom{d.H, d.D, 128, rup(d.D, 32), -1, c.lay.pl_w1};                 // W1 [H][D]
        case PL_W11: return PlaneGeom{d.D, d.H, rup(d.D, 128), 128, d.H, c.lay.pl_w11};              // [W11 | b11] [D][H + 1]
        case PL_D10: return PlaneGeom{d.B, d.H, rup(d.B, 256), 128, d.H, c.lay.pl_d10};              // [d10 | 1] [B][H + 1]
        default:     return PlaneGeom{d.B, d.H, rup(d.B, 256), 128, -1, c.lay.pl_dz1};               // dZ1 [B][H]
    }
}
static void use_planes(const Ctx& c, Operand& o, int kind) {
    const PlaneGeom g = plane_geom(c, kind);
    o.pl = reinterpret_cast<const unsigned short*>(c.ws + g.ws_off);
    o.pl_plane = (int64_t)g.Rp * g.Cp; o.pl_arm = 3 * o.pl_plane; o.pl_ld = g.Cp;
}
// bf16 storage (Plan::narrow): slice 0 of a plane set IS the matrix rounded to bf16; the bf16 engine reads the operand from it in
// sixteen-byte pieces, like x (half the bytes of fp32).  whole: rows and K become the planes' zero-padded extents (K-major).
// Returns the arm stride in FLOATS of the kernels' pointer arithmetic (the planes' elements are two bytes).
static int64_t read_slice0_bf16(const Ctx& c, Operand& o, int kind, bool whole = false) {
    const PlaneGeom g = plane_geom(c, kind);
    o.ptr = reinterpret_cast<const float*>(c.ws + g.ws_off); o.ld = g.Cp; o.src16 = 1;
    if (whole) { o.rows = g.Rp; o.K = g.Cp; }
    return 3 * (int64_t)g.Rp * g.Cp / 2;
}
static SplitJob plane_job(const Ctx& c, int kind, const float* src, int64_t ld, int64_t src_arm, const float* col_src = nullptr, int64_t col_arm = 0) {
    const PlaneGeom g = plane_geom(c, kind);
    return SplitJob{src, ld, src_arm, g.R, g.C, g.Rp, g.Cp, g.ones_col, reinterpret_cast<unsigned short*>(c.ws + g.ws_off),
                    3 * (int64_t)g.Rp * g.Cp, col_src, col_arm};
}
static int launch_presplit(hipStream_t s, int A, const SplitJob* jobs, int n, const XbitsJob* xb = nullptr) {
    SplitJobs js{};
    if (xb) js.xb = *xb;
    js.n = n;
    for (int i = 0; i < n; ++i) {   // a job gets the blocks its size asks for (small-layer planes: 8, W11: 320)
        js.j[i] = jobs[i];
        js.first[i + 1] = js.first[i] + (int)imin64(1024, cdiv64((int64_t)jobs[i].Rp * (jobs[i].Cp / 8), 256));
    }
    hipLaunchKernelGGL(k_presplit, dim3(js.xb.blocks + js.first[n], 1, A), dim3(256), 0, s, js);
    HIP_LAUNCH_CHECK("k_presplit");
    return 0;
}

// The small layers' weight planes for the chain kernels (Layout::pl_small): slot s holds [N][K] of fc2..fc5 (0..3) and
// fc6..fc10 (4..8), slot 9 + s the same layer as [K][N] for the backward chain (its contraction runs over N)
static SplitJob small_plane_job(const Ctx& c, const float* params, int s, bool transposed) {
    const int H = c.d.H, L = c.d.L, CS = c.d.C + c.d.S;
    const int ti[PL_SMALL_LAYERS] = {2, 4, 6, 8, 16, 18, 20, 22, 24};                    // parameter tensor index of the weight
    const int nn[PL_SMALL_LAYERS] = {H, H, H, L, L, H, H, H, H}, kk[PL_SMALL_LAYERS] = {H, H, H, H, CS, L, H, H, H};
    unsigned short* base = reinterpret_cast<unsigned short*>(c.ws + c.lay.pl_small);
    return SplitJob{params + c.po.o[ti[s]], kk[s], c.po.per_arm, transposed ? kk[s] : nn[s], transposed ? nn[s] : kk[s], 128, 128, -1,
                    base + (int64_t)(transposed ? PL_SMALL_LAYERS + s : s) * 3 * 128 * 128, (int64_t)PL_SMALL_SLOTS * 3 * 128 * 128,
                    nullptr, 0, transposed ? 1 : 0};
}

// Write slice planes from the parameters -- one small launch ahead of the kernels that copy them into LDS: at the head of a
// forward pass W1 and [W11 | b11] (fp32x3 engine, bf16 storage) and the small layers' weights (Plan::chain_planes), at the
// head of a backward pass that is its own call the small layers' weights alone.
int launch_x3_planes(const Ctx& c, const float* params, bool head, const mmvae_noise* nz) {
    const Plan& p = c.plan;
    const mmvae_dims& d = c.d;
    // ZERO_PRESPLIT (the head of a training step's forward pass, dropout on): this launch also makes the keep-mask and zeroes
    // the loss partial slots and the forward accumulator sets -- k_make_xbits' work (launch_forward_zero) without its launch
    XbitsJob xb{};
    const bool xbits = head && p.zero == ZERO_PRESPLIT;
    if (xbits) {
        xb.nz = make_noise_dev(nz, c.h);
        xb.A = d.A; xb.B = d.B; xb.D = d.D; xb.wpr = cdiv(d.D, 32);
        xb.bits = reinterpret_cast<uint32_t*>(c.ws + c.lay.xbits);
        xb.blocks = (int)imin64(2048, cdiv64((int64_t)d.B * cdiv(xb.wpr, xbits_words_per_thread(xb.nz)), 256));
        xb.zero_p = c.ws + c.lay.fc11_part;
        xb.zero_n4 = (int)(c.fwd_zero_floats() / 4);
        if (p.rowmap) {
            xb.rows = c.x_rows; xb.map = reinterpret_cast<unsigned*>(c.ws + c.lay.rowmap);
            xb.rows_ld = c.x_ld; xb.n_rows = c.x_nrows;
        }
    }
    SplitJob jobs[24];
    int n = 0;
    // (narrow, the bf16 configuration on bf16 storage: slice 0 of W1's planes IS bf16(W1) -- fc1 reads its narrow operand from
    // it in sixteen-byte pieces of eight elements, like x, instead of fp32 rounded by every block tile (half the bytes) -- and
    // slice 0 of [W11 | b11]'s planes is bf16(W11) for the fused fc11 kernel (the bias column meets a zero of d10))
    if (head && (p.big == GEMM_X3 || p.narrow)) {
        jobs[n++] = plane_job(c, PL_W1, params + c.po.o[0], d.D, c.po.per_arm);
        jobs[n++] = plane_job(c, PL_W11, params + c.po.o[26], d.H, c.po.per_arm, params + c.po.o[27], c.po.per_arm);   // bias: column fc_dim
    }
    if (p.chain_planes)
        for (int s = 0; s < PL_SMALL_LAYERS; ++s) {
            jobs[n++] = small_plane_job(c, params, s, false);
            jobs[n++] = small_plane_job(c, params, s, true);
        }
    return launch_presplit(c.stream, d.A, jobs, n, xbits ? &xb : nullptr);
}

// Decode: the planes its kernels read and nothing else -- fc6..fc10 for the chain kernels' fp32x3 form (forward slots only)
// and [W11 | b11] for k_fc11_out (no W1, no transposed slots, no keep-mask: launch_x3_planes' head launch makes all of those)
int launch_dec_planes(const Ctx& c, const float* params) {
    const Plan& p = c.plan;
    const mmvae_dims& d = c.d;
    SplitJob jobs[6];
    int n = 0;
    if (p.fc11 == FC11_OUT_X3 || p.fc11 == FC11_OUT_BF16)
        jobs[n++] = plane_job(c, PL_W11, params + c.po.o[26], d.H, c.po.per_arm, params + c.po.o[27], c.po.per_arm);
    if (p.chain_planes)
        for (int s = PL_SMALL_DEC0; s < PL_SMALL_LAYERS; ++s) jobs[n++] = small_plane_job(c, params, s, false);
    return n ? launch_presplit(c.stream, d.A, jobs, n) : 0;
}

int launch_fc11_out_bf16(const Ctx& c, float* x_rec) {
    const mmvae_dims& d = c.d;
    Operand w{}, dp{};
    use_planes(c, w, PL_W11); use_planes(c, dp, PL_D10);
    Fc11OutArgs a{};
    a.wpl = w.pl; a.w_plane = w.pl_plane; a.w_arm = w.pl_arm;
    a.dpl = dp.pl; a.d_plane = dp.pl_plane; a.d_arm = dp.pl_arm;
    a.out = x_rec;
    a.B = d.B; a.D = d.D;
    // gene splits: the smallest count whose grid fills whole rounds of the CUs to >= 90 % (one workgroup per CU at fp32x3's
    // register use, two at bf16's), at most one piece of 32 genes per split
    const bool x3 = c.plan.fc11 == FC11_OUT_X3;
    const int blocks = cdiv(d.B, 128) * d.A, slots = (x3 ? 1 : 2) * 256, cap = min(64, cdiv(d.D, 32));
    int ks = 1;
    double best = 0.0;
    for (int k = 1; k <= cap; ++k) {
        const int nwg = blocks * k;
        const double eff = (double)nwg / (double)(cdiv(nwg, slots) * slots);
        if (nwg >= slots && eff >= 0.9) { ks = k; break; }
        if (eff > best + 1e-9) { best = eff; ks = k; }
    }
    a.KS = ks;
    const dim3 grid(cdiv(d.B, 128), ks, d.A);
    if (x3) hipLaunchKernelGGL((k_fc11_out<3, 7>), grid, dim3(256), 0, c.stream, a);
    else hipLaunchKernelGGL((k_fc11_out<1, 8>), grid, dim3(256), 0, c.stream, a);
    HIP_LAUNCH_CHECK("k_fc11_out");
    return 0;
}

// x [cell][gene] as a GEMM operand, K-major for fc1 (k = gene) or K-minor for dW1 (x~, k = cell), with what the call attaches:
// the keep-mask words under input dropout, the row map when the batch is rows of the resident matrix (mmvae_train_step_rows),
// and under it the bf16 engine's bf16 copy (bf16 storage).  *arm, *bits_arm: arm strides of the matrix (floats) / the mask words.
static Operand x_operand(const Ctx& c, const float* x, int64_t xs, bool minor, int64_t* arm, int64_t* bits_arm) {
    const mmvae_dims& d = c.d;
    Operand o = minor ? kminor(x, d.D, d.D, d.B) : kmajor(x, d.D, d.B, d.D);
    if (c.dropout()) { o.bits = reinterpret_cast<const uint32_t*>(c.ws + c.lay.xbits); o.wpr = cdiv(d.D, 32); }
    if (c.plan.rowmap) { o.rowmap = reinterpret_cast<const unsigned*>(c.ws + c.lay.rowmap); o.nrec = c.x_nrows * c.x_ld; o.map_n = d.B; }
    if (c.plan.rowmap && c.plan.big != GEMM_X3 && c.x16) { o.ptr = reinterpret_cast<const float*>(c.x16); o.src16 = 1; }
    *arm = xs; *bits_arm = (int64_t)d.B * o.wpr;
    return o;
}

// The compiled instantiations of the two slab GEMM kernels by what their template arguments mean: engine, orientations, SHARE
// (fp32x3: the two tiles of a block share 1 = A, 2 = B), IDX (1 / 2: A / B through its row map), S16 (bit 0 / 1: A / B is bf16 in memory),
// MASK (the kernel requests x~'s keep-mask words: fp32x3 exactly when the operand has a mask; the bf16 engine's masked forms also
// take an x without one)
typedef void (*GemmKernel)(const GemmArgs);
struct SlabVariant { bool x3, aminor, bminor; int share, idx, s16, mask; GemmKernel kernel; };
#define BF16_GEMM(AMINOR, BMINOR, IDX, S16, MASK) SlabVariant{false, AMINOR, BMINOR, 0, IDX, S16, MASK, k_bf16_gemm<AMINOR, BMINOR, IDX, S16, MASK != 0>}
#define X3_GEMM(AMINOR, BMINOR, SHARE, IDX, MASK) SlabVariant{true, AMINOR, BMINOR, SHARE, IDX, 0, MASK, k_x3_gemm<AMINOR, BMINOR, SHARE, IDX, MASK != 0>}
static const SlabVariant slab_variants[] = {
    // fc1 -- x as it lies | through the row map | ... from its bf16 copy | ... and W1 from slice 0 of its planes
    BF16_GEMM(false, false, 0, 0, 1), BF16_GEMM(false, false, 1, 0, 1), BF16_GEMM(false, false, 1, 1, 1), BF16_GEMM(false, false, 1, 3, 1),
    // fp32x3 (one tile wide: the two tiles of a block share the W1 tile), x~ under its keep-mask | x without input dropout
    // (the row map exists only under input dropout -- Plan::rowmap --, so its form always carries the mask)
    X3_GEMM(false, false, 2, 0, 1), X3_GEMM(false, false, 2, 1, 1), X3_GEMM(false, false, 2, 0, 0),
    BF16_GEMM(false, true, 0, 0, 0),   // d(d10)
    // dW1 -- x~ in the same four forms, the last with dZ1 from slice 0 of its planes
    BF16_GEMM(true, true, 0, 0, 1), BF16_GEMM(true, true, 2, 0, 1), BF16_GEMM(true, true, 2, 2, 1), BF16_GEMM(true, true, 2, 3, 1),
    // fp32x3 (one tile high: they share the dZ1 tile), with and without the mask
    X3_GEMM(true, true, 1, 0, 1), X3_GEMM(true, true, 1, 2, 1), X3_GEMM(true, true, 1, 0, 0),
    // dW11 -- fp32 operands | on a bf16 dZ11 | fp32x3 (one tile wide: they share the [d10 | 1] tile)
    BF16_GEMM(true, true, 0, 0, 0), BF16_GEMM(true, true, 0, 1, 0), X3_GEMM(true, true, 2, 0, 0),
};
#undef BF16_GEMM
#undef X3_GEMM
// Launch the slab GEMM g on the plan's engine.  The kernel follows from the operands as they were built -- orientation, row
// map, bf16 source -- and from `share` (fp32x3 only); a combination that is not compiled is an error, not another kernel.
static int launch_slab_gemm(const Ctx& c, const GemmArgs& g, int share, dim3 grid, const char* what) {
    const bool x3 = c.plan.big == GEMM_X3, aminor = g.a.kminor != 0, bminor = g.b.kminor != 0;
    const int idx = (g.a.rowmap ? 1 : 0) | (g.b.rowmap ? 2 : 0), s16 = (g.a.src16 ? 1 : 0) | (g.b.src16 ? 2 : 0);
    if (!x3) share = 0;
    // fp32x3: the shared operand comes from its slice planes (ones column included); only the other one is read as fp32
    const Operand& f = share == 1 ? g.b : g.a;
    if (x3 && (!(share == 1 ? g.a : g.b).pl || (share == 1 ? g.a : g.b).bits || f.ones_row >= 0)) {
        set_error("%s: k_x3_gemm takes the shared operand as slice planes and masks / extends neither it nor the other by a ones row", what);
        return MMVAE_E_LAUNCH;
    }
    // bf16 engine: only B of the K-minor x K-minor forms without a row map compiles the ones row (k_bf16_gemm: BONES)
    if (!x3 && (g.a.ones_row >= 0 || (g.b.ones_row >= 0 && !(aminor && bminor && idx == 0)))) {
        set_error("%s: k_bf16_gemm extends only the B operand of a k-minor x k-minor product without a row map by a ones row", what);
        return MMVAE_E_LAUNCH;
    }
    // bf16 engine: the mask belongs to x~, which is A of the k-major x k-major product (fc1) or B of a k-minor x k-minor one (dW1)
    if (!x3 && ((g.a.bits && (aminor || bminor)) || (g.b.bits && !(aminor && bminor)))) {
        set_error("%s: k_bf16_gemm takes a keep-mask on A of a k-major x k-major or on B of a k-minor x k-minor product only", what);
        return MMVAE_E_LAUNCH;
    }
    const int mask = (x3 ? f.bits != nullptr : g.a.bits || g.b.bits) ? 1 : 0;
    // the exact form first; an unmasked x of the bf16 engine (x_drop = 0) also runs on the masked form of its product
    for (int pass = 0; pass < (x3 ? 1 : 2); ++pass)
        for (const SlabVariant& v : slab_variants)
            if (v.x3 == x3 && v.aminor == aminor && v.bminor == bminor && v.share == share && v.idx == idx && v.s16 == s16 &&
                (pass == 0 ? v.mask == mask : v.mask >= mask)) {
                hipLaunchKernelGGL(v.kernel, grid, dim3(x3 ? 512 : 256), 0, c.stream, g);
                HIP_LAUNCH_CHECK(what);
                return 0;
            }
    set_error("%s: no %s kernel for A k-%s, B k-%s, share %d, row map %d, bf16 source %d, mask %d", what, x3 ? "k_x3_gemm" : "k_bf16_gemm",
              aminor ? "minor" : "major", bminor ? "minor" : "major", share, idx, s16, mask);
    return MMVAE_E_LAUNCH;
}
// its grid.  fp32x3: a block carries two 128-row tiles of the GEMM's long side (`paired` rows); bf16: tiles_m x tiles_n
static dim3 slab_grid(const Ctx& c, const GemmArgs& g, int paired) {
    return dim3(c.plan.big == GEMM_X3 ? cdiv(cdiv(paired, BT), 2) : cdiv(g.M, BT) * cdiv(g.N, BT), g.KS, g.A);
}

int launch_fc1_fwd_bf16(const Ctx& c, const float* params, const float* x, int64_t xs) {
    const mmvae_dims& d = c.d;
    GemmArgs g{};
    g.a = x_operand(c, x, xs, false, &g.a_arm, &g.a_bits_arm);
    g.b = kmajor(params + c.po.o[0], d.D, d.H, d.D); g.b_arm = c.po.per_arm;
    if (c.plan.big == GEMM_X3) use_planes(c, g.b, PL_W1);
    else if (g.a.src16 && c.plan.narrow) g.b_arm = read_slice0_bf16(c, g.b, PL_W1);   // [128][rup(D, 32)] bf16, zero rows beyond H
    g.M = d.B; g.N = d.H; g.K = d.D; g.KS = c.lay.sp.ks_fc1; g.A = d.A;
    g.so = SlabOut{c.ws + c.lay.fc1_slab, (int64_t)d.A * d.B * NP, (int64_t)d.B * NP, NP, d.B, d.H};
    return launch_slab_gemm(c, g, 2, slab_grid(c, g, d.B), "k_bf16_gemm<fc1>");
}

// what the fc11 kernels of both engines share: [d10 | W11^T] operands, the gene split, loss / dZ11 / x_rec outputs
static GemmArgs fc11_args(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    GemmArgs g{};
    g.a = kmajor(c.ws + L.Dk[4], d.H, d.B, d.H);          // d10 [B][H]
    g.b = kmajor(params + c.po.o[26], d.H, d.D, d.H);      // W11 [D][H]
    g.M = d.B; g.N = d.D; g.K = d.H; g.KS = L.sp.ks_gd10; g.A = d.A; g.n11 = L.n11;
    g.fo = Fc11Out{params + c.po.o[27], x, c.ws + L.DZ11, x_rec, c.ws + L.fc11_part, c.fc11_coef(), d.B, d.D, nullptr, 0};
    if (c.plan.rowmap) {
        g.fo.xmap = reinterpret_cast<const unsigned*>(c.ws + L.rowmap);
        g.fo.x_nrec = c.x_nrows * c.x_ld;
    }
    g.fo_arm = (int64_t)d.B * d.D;
    g.fo_x_arm = xs;
    return g;
}
static SlabOut gd10_slab(const Ctx& c) {
    const mmvae_dims& d = c.d;
    return SlabOut{c.ws + c.lay.GD10_slab, (int64_t)d.A * d.B * d.H, (int64_t)d.B * d.H, d.H, d.B, d.H};
}

// fp32x3: only the fused train-step kernel exists in this engine (fc_dim + 1 <= 112, 128 cells per block fit the
// loss-partial slots, no x_rec); everything else runs the fp32 matrix-instruction kernels (Plan::fc11)
int launch_fc11_x3(const Ctx& c, const float* params, const float* x, int64_t xs) {
    const mmvae_dims& d = c.d;
    GemmArgs g = fc11_args(c, params, x, xs, nullptr);
    use_planes(c, g.b, PL_W11);
    use_planes(c, g.a, PL_D10);
    g.so = gd10_slab(c);
    // (fc11_fork_rides implies FC11_X3 or FC11_BF16 with fc11_grad, i.e. this launch or k_bf16_fc11g below)
    launch_k(c, c.plan.fc11_fork_rides ? c.ev(EV_FORK) : nullptr, k_x3_fc11g, dim3(cdiv(d.B, 128), g.KS, d.A), dim3(256), 0, g);
    HIP_LAUNCH_CHECK("k_x3_fc11g");
    return 0;
}

int launch_fc11_bf16(const Ctx& c, const float* params, const float* x, int64_t xs, float* x_rec, int need_grad) {
    const mmvae_dims& d = c.d;
    if (int rc = zero_fc11_part(c)) return rc;
    if (!fc11_slots_fit(c.lay, d.B)) { set_error("fc11 bf16: loss partial slots"); return MMVAE_E_LAUNCH; }
    GemmArgs g = fc11_args(c, params, x, xs, x_rec);
    g.a_arm = (int64_t)d.B * d.H;
    g.b_arm = c.po.per_arm;
    g.bias_arm = c.po.per_arm;
    const dim3 grid(cdiv(d.B, BT), g.KS, d.A);
    // forward for gradients without x_rec (the train step, mmvae_forward(need_grad) for backward): one fused kernel that
    // also writes d(d10); with x_rec wanted two kernels (launch_gd10_bf16)
    if (!(need_grad && !x_rec)) {
        hipLaunchKernelGGL(k_bf16_fc11, grid, dim3(256), 0, c.stream, g);
        HIP_LAUNCH_CHECK("k_bf16_fc11");
        return 0;
    }
    g.so = gd10_slab(c);
    // (fc11_fork_rides implies FC11_BF16 with fc11_grad -- need_grad without x_rec --, i.e. one of these three launches)
    const hipEvent_t fork = c.plan.fc11_fork_rides ? c.ev(EV_FORK) : nullptr;
    const bool s16 = c.plan.dz11_bf16;
    if (s16) {   // bf16 storage: x from its bf16 copy, dZ11 written as bf16 (dW11 reads it that way)
        g.fo.x = reinterpret_cast<const float*>(c.x16);
        g.fo_arm = (int64_t)d.B * d.D / 2;          // (arm stride of dZ11 in floats: B * D two-byte elements)
        // W11 from slice 0 of its planes (launch_x3_planes): all of [rup(D, 128)][128] bf16
        if (c.plan.narrow) g.b_arm = read_slice0_bf16(c, g.b, PL_W11, true);
    }
    // the compiled k_bf16_fc11g<S16, W16>, [S16: as above][W16: W11 is bf16 in memory]
    static const GemmKernel variants[2][2] = {{k_bf16_fc11g<false, false>, nullptr},
                                              {k_bf16_fc11g<true, false>, k_bf16_fc11g<true, true>}};
    const GemmKernel kernel = variants[s16][g.b.src16 != 0];
    if (!kernel) { set_error("k_bf16_fc11g: no kernel for a bf16 W11 beside an fp32 x"); return MMVAE_E_LAUNCH; }
    launch_k(c, fork, kernel, grid, dim3(256), 0, g);
    HIP_LAUNCH_CHECK("k_bf16_fc11g");
    return 0;
}

int launch_gd10_bf16(const Ctx& c, const float* params) {
    const mmvae_dims& d = c.d;
    GemmArgs g{};
    g.a = kmajor(c.ws + c.lay.DZ11, d.D, d.B, d.D);        // dZ11 [B][D], k = gene
    g.a_arm = (int64_t)d.B * d.D;
    g.b = kminor(params + c.po.o[26], d.H, d.H, d.D);      // W11 [D][H] read as B[n = h][k = j]
    g.b_arm = c.po.per_arm;
    g.M = d.B; g.N = d.H; g.K = d.D; g.KS = c.lay.sp.ks_gd10; g.A = d.A;
    g.so = gd10_slab(c);
    // (FC11_BF16 implies GEMM_BF16: there is no fp32x3 form of this product, and on that engine the lookup would say so)
    return launch_slab_gemm(c, g, 0, slab_grid(c, g, 0), "k_bf16_gemm<gd10>");
}

// dW1[h][d] = sum_b dZ1[b][h] x~[b][d]
int launch_dw1_bf16(const Ctx& c, const float* x, int64_t xs) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    GemmArgs g{};
    g.a = kminor(c.ws + L.DZ[1], d.H, d.H, d.B); g.a_arm = (int64_t)d.B * d.H;
    g.b = x_operand(c, x, xs, true, &g.b_arm, &g.b_bits_arm);
    if (c.plan.big == GEMM_X3) use_planes(c, g.a, PL_DZ1);
    else if (g.b.src16 && c.plan.narrow && c.plan.dz1_in_apply) g.a_arm = read_slice0_bf16(c, g.a, PL_DZ1);   // (k_bn_bwd_apply wrote them)
    g.M = d.H; g.N = d.D; g.K = d.B; g.KS = L.sp.ks_dw; g.A = d.A;
    g.so = SlabOut{c.ws + L.dw1_slab, (int64_t)d.A * d.H * d.D, (int64_t)d.H * d.D, d.D, d.H, d.D};
    return launch_slab_gemm(c, g, 1, slab_grid(c, g, d.D), "k_bf16_gemm<dW1>");
}

// [dW11 | db11][j][h] = sum_b dZ11[b][j] [d10 | 1][b][h]
int launch_dw11_bf16(const Ctx& c) {
    const mmvae_dims& d = c.d;
    const Layout& L = c.lay;
    GemmArgs g{};
    g.a = kminor(c.ws + L.DZ11, d.D, d.D, d.B); g.a_arm = (int64_t)d.B * d.D;
    g.b = kminor(c.ws + L.Dk[4], d.H, d.H, d.B); g.b_arm = (int64_t)d.B * d.H;
    g.b.ones_row = d.H;                                      // logical row H (not in memory) reads 1: the bias gradient
    if (c.plan.big == GEMM_X3) use_planes(c, g.b, PL_D10);
    else if (c.plan.dz11_bf16) { g.a.src16 = 1; g.a_arm /= 2; }   // bf16 storage: this step's fused fc11 kernel wrote dZ11 as bf16
    g.M = d.D; g.N = d.H + 1; g.K = d.B; g.KS = L.sp.ks_dw11; g.A = d.A;
    g.so = SlabOut{c.ws + L.dw11_slab, (int64_t)d.A * d.D * DW11_LD, (int64_t)d.D * DW11_LD, DW11_LD, d.D, d.H + 1};
    return launch_slab_gemm(c, g, 2, slab_grid(c, g, d.D), "k_bf16_gemm<dW11>");
}

int launch_dw_small_x3(const Ctx& c, const TnDescs& ts, int nsel) {
    const int KS = c.lay.sp.ks_small;
    hipLaunchKernelGGL(k_x3_small, dim3(cdiv(nsel * c.d.A, 2), KS), dim3(512), 0, c.stream, ts, nsel, c.d.A, c.d.B, KS);
    HIP_LAUNCH_CHECK("k_x3_small");
    return 0;
}

}  // namespace mmvae
