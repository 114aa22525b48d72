// bitslice.hip -- "is this window within Hamming distance r of the consensus" for EVERY window of the packed reads, bit-sliced
// over positions: 32 windows per thread at once instead of one funnel-shifted window at a time.
//
// Used by the occurrence scan (get_motif_occurence, motif_discovery.py:1422-1477 -- BASELINE config C5) and by masking
// (mask_input, kmer_count.py:580-610), k <= 16.  Both need, per window, only the predicate d <= r (the scan then evaluates the
// few hit windows exactly to find each read's minimum: scan_reads.hip).  The per-window formulation (scan_nibble_kernel /
// mask_flag_packed_kernel in scan_wide.hip: alignbit, shift, xor, 2-bit popcount, compare per window and strand: ~21 vector
// instructions per window, VALU-issue bound at 0.85 ms per consensus on the C3 reads) is replaced by:
//
//   * bit planes of the reads, built once per upload: planes[2w] = H, planes[2w + 1] = L for the 32 positions of word w (groups
//     2w, 2w + 1), H / L = the high / low bit of every base code, first position most significant (same order as the invalid mask);
//   * a thread takes 32 positions: H, L (and the following 32 for the window tails).  For consensus base j the mismatch plane
//     over the 32 windows is M_j = ((H << j) ^ CH_j) | ((L << j) ^ CL_j) with CH_j / CL_j = 0 or ~0 (scalar): 2 funnel shifts
//     shared by both strands + 3 logic ops per strand;
//   * the K mismatch planes are added bit-sliced by a carry-save tree of two-instruction full adders (compile-time K: ~1.6 ops
//     per plane) into a 4..5-bit counter per window, and "count > r" is the carry out of adding the constant 2^B - 1 - r (one
//     majority per counter bit);
//   * hit = (le_fwd | le_rc) for valid windows; a window that touches an invalid position has the reference's all-ones hash
//     ("compared like any value"), i.e. the same distance d_inv for all of them: hit = (d_inv <= r), a scalar.
// ~3.5 vector instructions per window at k = 8 with both strands, ~5.5 at k = 14 (r03's ripple-adder tree: 5.2 / 8.5), and the intermediate shrinks from 0.56 B
// (nibble + minimum) to 0.125 B (one bit) per position.
#include "common.h"
#include "scan_internal.h"

namespace {

constexpr int BS_TPB = 256;

// ---- planes -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t squeeze_even_bits(uint32_t x) {   // bits 30, 28, ..., 0 -> bits 15..0, order kept
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
// thread = one 32-position word: groups 2w, 2w + 1 (the array holds an even number of groups) -> planes[2w] = H, planes[2w + 1] = L
__global__ __launch_bounds__(BS_TPB) void planes_kernel(const uint32_t *__restrict__ codes, int64_t n_words, uint32_t *__restrict__ planes) {
    const int64_t w = (int64_t)blockIdx.x * BS_TPB + threadIdx.x;
    if (w >= n_words) return;
    const uint2 c = *reinterpret_cast<const uint2 *>(codes + 2 * w);
    uint2 o;
    o.x = (squeeze_even_bits(c.x >> 1) << 16) | squeeze_even_bits(c.y >> 1);
    o.y = (squeeze_even_bits(c.x) << 16) | squeeze_even_bits(c.y);
    *reinterpret_cast<uint2 *>(planes + 2 * w) = o;
}

// ---- bit-sliced counters --------------------------------------------------------------------------------------------
// The K mismatch planes of a strand are counted by a carry-save tree of full adders, each TWO instructions on gfx950
// (v_bitop3_b32: sum = a ^ b ^ c, carry = majority): planes of equal weight are taken three at a time until one is left -- the
// count's bit of that weight -- and the carries form the next weight's planes.  K = 14: 10 full adders + 1 half adder = 22
// instructions (the r03 balanced tree of ripple adders: 46), K = 8: 13.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }
constexpr int bits_for(int n) {   // bits that hold 0..n
    int b = 0;
    while ((1 << b) <= n) ++b;
    return b;
}
// N planes of one weight in cur[0 .. N) -> the count's bit of that weight (returned) and N / 2 carry planes in nxt[0 .. N / 2)
template <int N>
__device__ __forceinline__ uint32_t csa_level(uint32_t (&cur)[16], uint32_t (&nxt)[16]) {
    if constexpr (N == 0) return 0u;
    constexpr int FA = (N - 1) / 2;
#pragma unroll
    for (int it = 0; it < FA; ++it) {                                       // live planes: cur[0 .. N - 2 it)
        const int top = N - 2 * it - 1;
        const uint32_t x = cur[top], y = cur[top - 1], z = cur[top - 2];
        cur[top - 2] = xor3(x, y, z);
        nxt[it] = maj3(x, y, z);
    }
    if constexpr (N >= 2 && N % 2 == 0) {                                   // two planes left: half adder
        const uint32_t x = cur[0], y = cur[1];
        cur[0] = x ^ y;
        nxt[FA] = x & y;
    }
    return cur[0];
}
// windows whose mismatch count over the K planes exceeds r: the carry out of count + (2^B - 1 - r), r clamped to 2^B - 1
// (r >= 0: the callers drop entries with a negative radius, which match nothing).  Bit b of that constant as a scalar 0 / ~0:
// carry' = majority(count_b, carry, const_b) -- one instruction per counter bit.
template <int K>
__device__ __forceinline__ uint32_t count_greater_than(const uint32_t (&m)[K], int r) {
    constexpr int B = bits_for(K);
    uint32_t l0[16], l1[16], l2[16], l3[16], l4[16], cnt[5];
#pragma unroll
    for (int j = 0; j < K; ++j) l0[j] = m[j];
    cnt[0] = csa_level<K>(l0, l1);
    cnt[1] = csa_level<K / 2>(l1, l2);
    cnt[2] = csa_level<K / 4>(l2, l3);
    cnt[3] = csa_level<K / 8>(l3, l4);
    cnt[4] = csa_level<K / 16>(l4, l0);
    const int rr = r > (1 << B) - 1 ? (1 << B) - 1 : r;
    const uint32_t konst = (uint32_t)((1 << B) - 1 - rr);
    uint32_t carry = 0;
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const uint32_t kb = 0u - ((konst >> b) & 1u);
        carry = b == 0 ? (cnt[0] & kb) : maj3(cnt[b], carry, kb);
    }
    return carry;
}

// ---- hit bits of 32 windows per thread ------------------------------------------------------------------------------
struct HitCons {
    uint32_t fwd, rc;      // consensus codes (2 bits per base, first base most significant), rc used when two != 0
    int32_t radius;
    uint32_t two;          // also test the reverse-complement strand
    uint32_t inv_hit;      // ~0 when an invalid window (all-ones hash) lies within radius of this entry, else 0
};
struct HitTab {
    HitCons c[16];
    int n;
};

template <int K>
__device__ __forceinline__ uint32_t strand_gt(const uint32_t (&hs)[K], const uint32_t (&ls)[K], uint32_t code, int radius) {
    uint32_t m[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint32_t base = (code >> (2 * (K - 1 - j))) & 3u;          // scalar
        const uint32_t ch = 0u - (base >> 1), cl = 0u - (base & 1u);
        m[j] = (hs[j] ^ ch) | (ls[j] ^ cl);
    }
    return count_greater_than<K>(m, radius);
}

// ---- mismatch planes through the VGPR index mode ---------------------------------------------------------------------------
// (h ^ ch) | (l ^ cl) has four inputs, two of them the consensus base: as written above a mismatch plane costs the strand two
// instructions on top of the shared funnel shifts (3 per plane and strand in all).  The base only SELECTS one of four functions of
// (h, l): E_A = h | l, E_C = h | ~l, E_G = ~h | l, E_T = ~h | ~l -- "the base here is not b" for the 64 positions a thread holds,
// 8 instructions shared by every strand and table entry.  The mismatch plane of consensus position j is then the funnel shift by
// j of E_b with b = the consensus base, and gfx9's VGPR index mode lets a SCALAR pick the register: with
// s_set_gpr_idx_on / _idx (M0[7:0] = b, SRC0 and SRC1 relative) `v_alignbit_b32 m, v40, v44, 32 - j` reads v[40 + b], v[44 + b]:
// ONE vector instruction per plane and strand.  A thread carries TWO 32-window words (E planes in v40..v47 and v48..v55, pinned by
// explicit-register constraints), so that one scalar index change serves two vector instructions and the scalar unit, which
// issues beside the vector unit, stays the smaller stream.  Blocks hold 8 / 4 / 2 / 1 planes (an asm statement takes 30
// operands); every block leaves the index mode switched off.  M0 is not on the clobber lists: the compiler reserves it (it
// sets M0 itself right before the few instructions that read it) and rejects it there.
// HAZARD (measured, not in the ISA manual's table): a vector instruction issued right behind the s_set_gpr_idx_* that changes
// M0 can still see the OLD index -- without a wait state ~1 wave in 10^4 produced hit words of the wrong planes at C5 size, a
// different set of waves every run; with `s_nop 0` (one wait state, what the manual asks between an M0 write and s_movrel /
// LDS-add-TID / interp) none in repeated full-size runs.  KMAP_IDX_WAIT is two wait states (behind every index change and
// behind s_set_gpr_idx_off, whose successor is whatever the compiler schedules next); tests/test_gpu_fullsize.py holds the
// full-size comparison against the formulation without the index mode.
#define KMAP_IDX_WAIT "s_nop 1\n\t"
#define KMAP_IDX_WAIT_END "s_nop 1"      // the same distance between switching the mode off and the compiler's next vector instruction
typedef uint32_t EPlanes __attribute__((ext_vector_type(8)));   // {A, C, G, T} of word 0 (positions P .. P + 31), of word 1 (the next 32)
#define KMAP_E_INS "{v[40:47]}"(ea), "{v[48:55]}"(eb)
__device__ __forceinline__ EPlanes make_eplanes(uint32_t H, uint32_t L, uint32_t H2, uint32_t L2) {
    EPlanes e;                           // one instruction each (left to itself the compiler spent a v_not and a 64-bit move on some)
    e[0] = H | L, e[4] = H2 | L2;
    e[1] = __builtin_amdgcn_bitop3_b32(H, L, L, 0xF3), e[5] = __builtin_amdgcn_bitop3_b32(H2, L2, L2, 0xF3);      // a | ~b
    e[2] = __builtin_amdgcn_bitop3_b32(H, L, L, 0xCF), e[6] = __builtin_amdgcn_bitop3_b32(H2, L2, L2, 0xCF);      // ~a | b
    e[3] = __builtin_amdgcn_bitop3_b32(H, L, L, 0x3F), e[7] = __builtin_amdgcn_bitop3_b32(H2, L2, L2, 0x3F);      // ~(a & b)
    return e;
}
// plane 0 needs no shift: the selected word 0 itself
__device__ __forceinline__ void idx_plane0(const EPlanes &ea, const EPlanes &eb, uint32_t c0, uint32_t &ma, uint32_t &mb) {
    asm("s_set_gpr_idx_on %[c0], gpr_idx(SRC0)\n\t" KMAP_IDX_WAIT
        "v_mov_b32 %[a0], v40\n\t"
        "v_mov_b32 %[b0], v48\n\t"
        "s_set_gpr_idx_off\n\t" KMAP_IDX_WAIT_END
        : [a0] "=&v"(ma), [b0] "=&v"(mb)
        : [c0] "s"(c0), KMAP_E_INS);
}
// planes J0 .. J0 + N - 1 (J0 >= 1) of both words: m[j] = funnel shift of E_{c[j]} by j.  One text for the four block sizes: the
// first step switches the mode on, step i changes the index and shifts by one less (%[s] = 32 - J0), the end switches it off
#define KMAP_IDX_FIRST                                         \
    "s_set_gpr_idx_on %[c0], gpr_idx(SRC0,SRC1)\n\t" KMAP_IDX_WAIT \
    "v_alignbit_b32 %[a0], v40, v44, %[s]\n\t"                 \
    "v_alignbit_b32 %[b0], v48, v52, %[s]\n\t"
#define KMAP_IDX_NEXT(i)                                       \
    "s_set_gpr_idx_idx %[c" #i "]\n\t" KMAP_IDX_WAIT           \
    "v_alignbit_b32 %[a" #i "], v40, v44, %[s]-" #i "\n\t"     \
    "v_alignbit_b32 %[b" #i "], v48, v52, %[s]-" #i "\n\t"
#define KMAP_IDX_END "s_set_gpr_idx_off\n\t" KMAP_IDX_WAIT_END
#define KMAP_IDX_OUT(i) [a##i] "=&v"(ma[J0 + i]), [b##i] "=&v"(mb[J0 + i])
#define KMAP_IDX_IN(i) [c##i] "s"(c[J0 + i])
#define KMAP_IDX_TAIL [s] "n"(32 - J0), KMAP_E_INS
template <int J0>
__device__ __forceinline__ void idx_planes1(const EPlanes &ea, const EPlanes &eb, const uint32_t *c, uint32_t *ma, uint32_t *mb) {
    asm(KMAP_IDX_FIRST KMAP_IDX_END : KMAP_IDX_OUT(0) : KMAP_IDX_IN(0), KMAP_IDX_TAIL);
}
template <int J0>
__device__ __forceinline__ void idx_planes2(const EPlanes &ea, const EPlanes &eb, const uint32_t *c, uint32_t *ma, uint32_t *mb) {
    asm(KMAP_IDX_FIRST KMAP_IDX_NEXT(1) KMAP_IDX_END : KMAP_IDX_OUT(0), KMAP_IDX_OUT(1) : KMAP_IDX_IN(0), KMAP_IDX_IN(1), KMAP_IDX_TAIL);
}
template <int J0>
__device__ __forceinline__ void idx_planes4(const EPlanes &ea, const EPlanes &eb, const uint32_t *c, uint32_t *ma, uint32_t *mb) {
    asm(KMAP_IDX_FIRST KMAP_IDX_NEXT(1) KMAP_IDX_NEXT(2) KMAP_IDX_NEXT(3) KMAP_IDX_END
        : KMAP_IDX_OUT(0), KMAP_IDX_OUT(1), KMAP_IDX_OUT(2), KMAP_IDX_OUT(3)
        : KMAP_IDX_IN(0), KMAP_IDX_IN(1), KMAP_IDX_IN(2), KMAP_IDX_IN(3), KMAP_IDX_TAIL);
}
template <int J0>
__device__ __forceinline__ void idx_planes8(const EPlanes &ea, const EPlanes &eb, const uint32_t *c, uint32_t *ma, uint32_t *mb) {
    asm(KMAP_IDX_FIRST KMAP_IDX_NEXT(1) KMAP_IDX_NEXT(2) KMAP_IDX_NEXT(3) KMAP_IDX_NEXT(4) KMAP_IDX_NEXT(5) KMAP_IDX_NEXT(6) KMAP_IDX_NEXT(7) KMAP_IDX_END
        : KMAP_IDX_OUT(0), KMAP_IDX_OUT(1), KMAP_IDX_OUT(2), KMAP_IDX_OUT(3), KMAP_IDX_OUT(4), KMAP_IDX_OUT(5), KMAP_IDX_OUT(6), KMAP_IDX_OUT(7)
        : KMAP_IDX_IN(0), KMAP_IDX_IN(1), KMAP_IDX_IN(2), KMAP_IDX_IN(3), KMAP_IDX_IN(4), KMAP_IDX_IN(5), KMAP_IDX_IN(6), KMAP_IDX_IN(7), KMAP_IDX_TAIL);
}
#undef KMAP_IDX_FIRST
#undef KMAP_IDX_NEXT
#undef KMAP_IDX_END
#undef KMAP_IDX_OUT
#undef KMAP_IDX_IN
#undef KMAP_IDX_TAIL
#undef KMAP_E_INS
// windows of the two words whose distance to `code` exceeds the radius
template <int K>
__device__ __forceinline__ void strand_gt_idx(const EPlanes &ea, const EPlanes &eb, uint32_t code, int radius, uint32_t &gta, uint32_t &gtb) {
    uint32_t c[K], ma[K], mb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) c[j] = (code >> (2 * (K - 1 - j))) & 3u;   // scalar: the consensus base of plane j
    idx_plane0(ea, eb, c[0], ma[0], mb[0]);
    constexpr int R = K - 1;                                                // planes 1 .. K - 1 in blocks of 8, 4, 2, 1
    if constexpr (R >= 8) idx_planes8<1>(ea, eb, c, ma, mb);
    constexpr int J4 = 1 + (R & 8);
    if constexpr ((R & 4) != 0) idx_planes4<J4>(ea, eb, c, ma, mb);
    constexpr int J2 = J4 + (R & 4);
    if constexpr ((R & 2) != 0) idx_planes2<J2>(ea, eb, c, ma, mb);
    constexpr int J1 = J2 + (R & 2);
    if constexpr ((R & 1) != 0) idx_planes1<J1>(ea, eb, c, ma, mb);
    gta = count_greater_than<K>(ma, radius);
    gtb = count_greater_than<K>(mb, radius);
}

// the 64 positions from group g0 (even) on as bit planes, and the windows among the first 32 that touch an invalid position.
// Groups g0 .. g0 + 3 as two aligned pairs: g0 < the number of data groups, and the array holds an even number of groups of
// which at least the last two are all-invalid halo groups (kmap_packed_groups), so g0 + 3 is inside it.
template <int K>
__device__ __forceinline__ void load_word(const uint32_t *__restrict__ planes, const uint16_t *__restrict__ inval, int64_t g0, uint32_t &H,
                                          uint32_t &L, uint32_t &H2, uint32_t &L2, uint32_t &bad) {
    const uint2 pa = *reinterpret_cast<const uint2 *>(planes + g0), pb = *reinterpret_cast<const uint2 *>(planes + g0 + 2);
    const uint32_t ia = *reinterpret_cast<const uint32_t *>(inval + g0), ib = *reinterpret_cast<const uint32_t *>(inval + g0 + 2);
    H = pa.x, L = pa.y, H2 = pb.x, L2 = pb.y;
    // OR of the invalid flags of positions p .. p + K - 1 (doubling on the 64-bit stream); a little-endian pair of flag words has
    // the first group in its low half: rotate by 16
    // (32-bit halves: funnel shift + or for the upper, shift-or for the lower word -- no 64-bit shifts; the lower word's last step is
    // not needed)
    uint32_t hi = __builtin_amdgcn_alignbit(ia, ia, 16), lo = __builtin_amdgcn_alignbit(ib, ib, 16);
#pragma unroll
    for (int have = 1; have < K;) {
        const int step = (have <= K - have) ? have : K - have;
        hi |= __builtin_amdgcn_alignbit(hi, lo, 32 - step);
        have += step;
        if (have < K) lo |= lo << step;
    }
    bad = hi;
}
template <bool WORDS>
__device__ __forceinline__ void store_word(uint16_t *__restrict__ hit16, int64_t w, uint32_t hit, int64_t n) {
    const int64_t left = n - 32 * w;                                      // positions past the end do not exist
    if (left < 32) hit &= ~((1u << (32 - (int)left)) - 1u);
    if (WORDS) reinterpret_cast<uint32_t *>(hit16)[w] = hit;
    else *reinterpret_cast<uint32_t *>(hit16 + 2 * w) = (hit << 16) | (hit >> 16);   // little-endian halves: hit16[2 w] = windows 0..15
}

// hit16[g]: bit (15 - i) set when the window at position 16 g + i is within radius of any table entry (invalid windows: the
// entry's inv_hit).  Thread = word t = groups 2t, 2t + 1.  planes / inval are read up to group 2t + 3 (inside the array: see kmap_packed_groups).
// WORDS: store the 32 hit bits as ONE word, window i in bit 31 - i (hit32[t], the scan's per-read passes); otherwise as the
// two uint16 of the mask's coverage pass.
template <int K, bool WORDS>
__global__ __launch_bounds__(BS_TPB) void hits_planes_kernel(const uint32_t *__restrict__ planes, const uint16_t *__restrict__ inval,
                                                            int64_t n, HitTab tab, uint16_t *__restrict__ hit16) {
    const int64_t t = (int64_t)blockIdx.x * BS_TPB + threadIdx.x;
    if (32 * t >= n) return;
    uint32_t H, L, H2, L2, bad;
    load_word<K>(planes, inval, 2 * t, H, L, H2, L2, bad);
    uint32_t hs[K], ls[K];
    hs[0] = H;
    ls[0] = L;
#pragma unroll
    for (int j = 1; j < K; ++j) {
        hs[j] = __builtin_amdgcn_alignbit(H, H2, 32 - j);                 // bit (31 - i): base at position P + i + j
        ls[j] = __builtin_amdgcn_alignbit(L, L2, 32 - j);
    }
    uint32_t hit = 0;
    for (int c = 0; c < tab.n; ++c) {
        const HitCons e = tab.c[c];
        uint32_t gt = strand_gt<K>(hs, ls, e.fwd, e.radius);
        if (e.two) gt &= strand_gt<K>(hs, ls, e.rc, e.radius);           // within radius on either strand <=> not (both exceed)
        hit |= (~gt & ~bad) | (bad & e.inv_hit);
    }
    store_word<WORDS>(hit16, t, hit, n);
}

// The same through the index mode: a block takes 2 * BS_TPB consecutive words, thread i the words i and BS_TPB + i of them.
template <int K, bool WORDS>
__global__ __launch_bounds__(BS_TPB) void hits_planes_idx_kernel(const uint32_t *__restrict__ planes, const uint16_t *__restrict__ inval,
                                                                int64_t n, HitTab tab, uint16_t *__restrict__ hit16) {
    const int64_t wa = (int64_t)blockIdx.x * (2 * BS_TPB) + threadIdx.x;
    if (32 * wa >= n) return;
    const int64_t wb = wa + BS_TPB;
    const bool has_b = 32 * wb < n;                                       // otherwise: word a once more, not stored
    uint32_t H, L, H2, L2, bad_a, bad_b;
    load_word<K>(planes, inval, 2 * wa, H, L, H2, L2, bad_a);
    const EPlanes ea = make_eplanes(H, L, H2, L2);
    load_word<K>(planes, inval, 2 * (has_b ? wb : wa), H, L, H2, L2, bad_b);
    const EPlanes eb = make_eplanes(H, L, H2, L2);
    uint32_t hit_a = 0, hit_b = 0;
    for (int c = 0; c < tab.n; ++c) {
        const HitCons e = tab.c[c];
        uint32_t gta, gtb;
        strand_gt_idx<K>(ea, eb, e.fwd, e.radius, gta, gtb);
        if (e.two) {
            uint32_t ra, rb;
            strand_gt_idx<K>(ea, eb, e.rc, e.radius, ra, rb);
            gta &= ra;
            gtb &= rb;
        }
        hit_a |= (~gta & ~bad_a) | (bad_a & e.inv_hit);
        hit_b |= (~gtb & ~bad_b) | (bad_b & e.inv_hit);
    }
    store_word<WORDS>(hit16, wa, hit_a, n);
    if (has_b) store_word<WORDS>(hit16, wb, hit_b, n);
}

template <int K>
void launch_hits(const uint32_t *planes, const uint16_t *inval, int64_t n, const HitTab &tab, uint16_t *hit16, bool words,
                 hipStream_t st) {
    const char *v = getenv("KMAP_SCAN_PLANES");                          // "plain": the formulation without the index mode (tests compare the two)
    const bool idx = !(v && !strcmp(v, "plain"));
    const int64_t n_words = (n + 31) / 32;
    if (idx && words) hits_planes_idx_kernel<K, true><<<grid_for(n_words, 2 * BS_TPB), BS_TPB, 0, st>>>(planes, inval, n, tab, hit16);
    else if (idx) hits_planes_idx_kernel<K, false><<<grid_for(n_words, 2 * BS_TPB), BS_TPB, 0, st>>>(planes, inval, n, tab, hit16);
    else if (words) hits_planes_kernel<K, true><<<grid_for(n_words, BS_TPB), BS_TPB, 0, st>>>(planes, inval, n, tab, hit16);
    else hits_planes_kernel<K, false><<<grid_for(n_words, BS_TPB), BS_TPB, 0, st>>>(planes, inval, n, tab, hit16);
}

}  // namespace

// hit bits of all windows for up to 16 table entries (k <= 16); hit16: uint16[(n + 15) / 16 rounded up to even] in group order,
// or (words) uint32[(n + 31) / 32] with window i of word t in bit 31 - i
int kmap_bitslice_hits(const uint32_t *planes, const uint16_t *inval, int64_t n, int k, const uint64_t *cons, const int32_t *radius,
                       int n_cons, int revcom_pairs, uint16_t *hit16, bool words, hipStream_t st) {
    KMAP_REQUIRE(k >= 1 && k <= 16 && n_cons >= 1 && n_cons <= 16, "bitslice_hits: k / table size out of range");
    HitTab tab;
    memset(&tab, 0, sizeof tab);
    tab.n = n_cons;
    const uint32_t km = low_mask<uint32_t>(k);
    for (int c = 0; c < n_cons; ++c) {
        HitCons &e = tab.c[c];
        e.fwd = (uint32_t)cons[c] & km;
        e.rc = (uint32_t)host_revcom(e.fwd, k, k < 16);
        e.two = revcom_pairs ? 1u : 0u;
        e.radius = radius[c];
        e.inv_hit = host_invalid_dist(e.fwd, e.rc, k, revcom_pairs) <= e.radius ? ~0u : 0u;
    }
    switch (k) {
#define KMAP_BS_CASE(KK) case KK: launch_hits<KK>(planes, inval, n, tab, hit16, words, st); break;
        KMAP_BS_CASE(1) KMAP_BS_CASE(2) KMAP_BS_CASE(3) KMAP_BS_CASE(4) KMAP_BS_CASE(5) KMAP_BS_CASE(6) KMAP_BS_CASE(7) KMAP_BS_CASE(8)
        KMAP_BS_CASE(9) KMAP_BS_CASE(10) KMAP_BS_CASE(11) KMAP_BS_CASE(12) KMAP_BS_CASE(13) KMAP_BS_CASE(14) KMAP_BS_CASE(15) KMAP_BS_CASE(16)
#undef KMAP_BS_CASE
    }
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

extern "C" {

int kmap_pack_planes_dev(const uint32_t *codes_dev, int64_t n, uint32_t *planes_dev, void *stream) {
    KMAP_REQUIRE(n >= 0, "pack_planes: negative size");
    const int64_t ng = kmap_packed_groups(n);
    KMAP_REQUIRE(codes_dev && planes_dev, "pack_planes: null pointer");
    KMAP_REQUIRE((((uintptr_t)codes_dev | (uintptr_t)planes_dev) & 7u) == 0u, "pack_planes: codes / planes must be 8-byte aligned (whole arrays, not offsets into them)");
    planes_kernel<<<grid_for(ng / 2, BS_TPB), BS_TPB, 0, as_stream(stream)>>>(codes_dev, ng / 2, planes_dev);   // ng is even
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

}  // extern "C"
