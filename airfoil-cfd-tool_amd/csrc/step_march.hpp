// step_march.hpp — what every marching kernel (k_march3, step_march3.hpp / step_chain.hpp) shares: the classes of the window tiles, the
// bounce codes, the unit and parameter records, the vector and buffer helpers, the collision of S sites per lane, step 1 of a column and
// the host-side unit planners.
//
// A wave owns a WINDOW of 64 S rows (j, the fast axis; S sites per lane, one 8-byte vector per lane and direction — fp32 S = 2, fp64 S = 1)
// and marches along a UNIT of columns (i), advancing several lattice steps per pass with the intermediate levels held in registers.
// Every window-tile (column x, window w) has a class (k_classify_windows, wave ballots):
//     FAST = no solid site in its 3 x (64 S + 2) neighbourhood, SOLID = every own site solid, GENERAL = the rest;
//     a unit reads the classes of its columns once and dispatches per column on a scalar bit test.  GENERAL tiles read one word of solid
//     flags and one word of BOUNCE CODES per lane (bit k-1 = the upstream neighbour of direction k is solid; k_bounce_codes, once per mask
//     upload) in place of the reference's nine mask texel reads (html:324-334); the sites' own populations supply the bounced values.
//     The inlet (html:314-322) and outlet (html:301-312) columns are marched too: the outlet column NX-1 is emitted with column NX-2.
// Addressing: buffer instructions — one resource descriptor per lattice in scalar registers, ONE per-lane byte offset for all 18 streams,
// the plane/column part of every address is a scalar add.
// Every site is computed by exactly the arithmetic of k_step: results are bit-identical.
// (Round 2's two-step kernel lived here too; it was retired once k_march3 ran passes of every length on its own tables — DESIGN.md §7a.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "step_fast.hpp"

#ifndef WT_LOAD_AUX
#define WT_LOAD_AUX 2       // cache policy of the streamed lattice loads: nt (read once per pass)
#endif
#ifndef WT_STORE_AUX
#define WT_STORE_AUX 2      // cache policy of the lattice stores: nt (written once, read by the NEXT pass); measured 2-4.5 % faster than 0
#endif

namespace wt {

static constexpr int MARCH_MAX_CHUNK = 60;       // two-step tables: the unit length of round 2's two-step kernel (one ballot of class bits), kept so that their plans stay as they were
static constexpr int MARCH3_MAX_CHUNK = 124;     // three / four steps per pass: two ballots (ClassMask), columns ia-PAD .. ib+PAD-1 <= 128
// most columns a unit of a `depth`-step plan may hold (the planners' max_len; a four-step unit's class masks reach three columns beyond it)
static inline int march_max_len(int depth) { return depth == 4 ? MARCH3_MAX_CHUNK - 3 : (depth == 3 ? MARCH3_MAX_CHUNK : MARCH_MAX_CHUNK); }
// columns beyond either end of a unit of a `depth`-step pass whose classes it reads — its class masks cover ia-PAD .. ib+PAD-1 —, and that a chain
// block's footprint takes in: a four-step unit computes level 1 of three columns on either side, the others of (at most) two
__host__ __device__ constexpr int march_pad(int depth) { return depth == 4 ? 3 : 2; }

// classes of up to 128 consecutive columns of a window, one bit each (lane l of the first ballot <-> the first column + l, of the second + 64 + l)
struct ClassMask { unsigned long long lo, hi; };
__device__ __forceinline__ bool cm_bit(const ClassMask &m, int idx) { return (((idx < 64) ? (m.lo >> idx) : (m.hi >> (idx - 64))) & 1ULL) != 0; }

enum : uint8_t { WC_FAST = 0, WC_GENERAL = 1, WC_SOLID = 2 };

// window height = window pitch = 64 lanes x S sites
static inline int march_nwin(int ny, int win) { return (ny + win - 1) / win; }

// collision for either element type: fp32 with the division selected by FD (d2q9.hpp), fp64 always IEEE
static constexpr int MARCH_FD_CONTRACTED = 8;    // bit 3 of FD: the opt-in contracted collision (d2q9.hpp collide_contracted; fp32 only)
static constexpr int MARCH_FD_TWOOP = 16;        // bit 4 of FD: the two-operation division by tau (d2q9.hpp; fp32, proved per tau like the three-operation one)
static constexpr int MARCH_FD_OVL = 32;          // bit 5 of FD (k_march3): OVERLAPPING windows — no halo lines, no seam buffer (step_chain.hpp k_march3); not an arithmetic choice,
                                                 // carried in FD because every function of the marching loop already takes it
template <typename T, int FD>
__device__ __forceinline__ void collide_t(const T (&fin)[9], const FastDiv &fdv, T tau, T (&fo)[9], T &rho, T &ux, T &uy)
{
    if constexpr (sizeof(T) == 4 && (FD & MARCH_FD_CONTRACTED) != 0) collide_contracted(fin, fdv.rtau, fo, rho, ux, uy);
    else if constexpr (sizeof(T) == 4) collide_fd<(FD & 3), (FD & MARCH_FD_TWOOP) != 0>(fin, fdv, fo, rho, ux, uy);
    else if constexpr ((FD & 3) != 0) collide_fd64(fin, fdv, fo, rho, ux, uy);       // fp64: the four-operation division, guarded (d2q9.hpp)
    else collide<T>(fin, tau, fo, rho, ux, uy);
}

// ------------------------------------------------------------------------------------------------
// once per mask upload
// ------------------------------------------------------------------------------------------------
// wcls[w * ld + (x + 1)], x = -1 .. nxl (the two extra columns are FAST), ld = nxl + 2
// (window w = rows w * stride + off .. + win - 1: stride = win, off = 0 for windows that tile the column; overlapping windows: k_march3)
__global__ __launch_bounds__(256) void k_classify_windows(const uint8_t *__restrict__ mask, uint8_t *__restrict__ wcls, Geom g, int nwin, int win, int stride, int off)
{
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int ld = g.nxl + 2;
    if (tile >= (long)ld * nwin) return;
    const int w = (int)(tile / ld), x = (int)(tile % ld) - 1;
    uint8_t cls = WC_FAST;
    if (x >= 0 && x < g.nxl) {
        const int j0 = w * stride + off;
        const uint8_t *m = mask + g.pitch;
        int nb = 0, own_all = 1;
        for (int jj = j0 - 1 + lane; jj <= j0 + win; jj += 64) {
            if (jj < 0 || jj >= g.ny) continue;
            const int a = m[(long)(x - 1) * g.pitch + jj], b = m[(long)x * g.pitch + jj], c = m[(long)(x + 1) * g.pitch + jj];
            nb |= a | b | c;
            if (jj >= j0 && jj < j0 + win) own_all &= (b != 0);      // (rows outside the lattice — a window that overlaps its end — do not count)
        }
        const bool any_nb = __ballot(nb != 0) != 0ULL;
        const bool all_own = __ballot(own_all == 0) == 0ULL;
        cls = !any_nb ? WC_FAST : (all_own ? WC_SOLID : WC_GENERAL);
    }
    if (lane == 0) wcls[(long)w * ld + x + 1] = cls;
}

// bcode[x * pitch + j], bit k-1 set <=> site (x - ex_k, j - ey_k) is solid (k = 1..8); 0 on rows 0 / NY-1;
// 0xFF on solid sites
__global__ __launch_bounds__(256) void k_bounce_codes(const uint8_t *__restrict__ mask, uint8_t *__restrict__ bcode, Geom g)
{
    const uint8_t *m = mask + g.pitch;
    const long total = (long)g.nxl * g.pitch;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int x = (int)(t / g.pitch), j = (int)(t % g.pitch);
        unsigned code = 0;
        if (j < g.ny && m[(long)x * g.pitch + j]) code = 0xffu;       // a solid site "bounces" every direction: fin[k] = own[opp(k)]
        else if (j >= 1 && j < g.ny - 1) {
#pragma unroll
            for (int k = 1; k < 9; k++)
                if (m[(long)(x - ex_of(k)) * g.pitch + (j - ey_of(k))]) code |= 1u << (k - 1);
        }
        bcode[t] = (uint8_t)code;
    }
}

// ------------------------------------------------------------------------------------------------
// once per pass: the halo kernels' fall-back (k_halo3 / k_halo4, step_march3.hpp)
// ------------------------------------------------------------------------------------------------
// One lattice site, step 1 only, every branch of STEP_FS main() (html:283-360) in the reference's order —
// the arithmetic of site_general (kernels.hpp) with the relaxation of collide_t.
template <typename T, int FD>
__device__ __forceinline__ void site_step1(const T *__restrict__ s, const uint8_t *__restrict__ m, const Geom &g, int i, int j,
                                           const FastDiv &fdv, T tau, T U0, T (&out)[9])
{
    const long c = (long)i * g.pitch + j;
    const int gi = i + g.gi0;
    if (m[c]) {                                                    // html:287-294 solid
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = s[opp_of(k) * g.plane + c];
    } else if (gi == g.nx_g - 1) {                                 // html:301-312 outlet
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = s[k * g.plane + c - g.pitch];
    } else if (gi == 0 || j == g.ny - 1 || j == 0) {               // html:314-322 far field
        feq_all<T>(T(1), U0, T(0), out);
    } else {                                                       // html:324-359 interior fluid
        T fin[9], rho, ux, uy;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const long src = c - (long)ex_of(k) * g.pitch - ey_of(k);
            fin[k] = m[src] ? s[opp_of(k) * g.plane + c] : s[k * g.plane + src];
        }
        collide_t<T, FD>(fin, fdv, tau, out, rho, ux, uy);
    }
}

// ------------------------------------------------------------------------------------------------
// units
// ------------------------------------------------------------------------------------------------
struct MarchUnit { int ia, ib, w, flags; };      // marched columns [ia, ib), window; flags bit 0: emit the outlet column ib with column ib-1
enum { MU_OUTLET_AFTER = 1 };

template <typename T>
struct MarchParams {
    const T *fs;
    T *fd;
    T *macro;
    const uint8_t *mask;       // padded byte mask (column -1 first)
    const uint8_t *bcode;      // bounce codes, column 0 first
    const uint8_t *wcls;       // window-tile classes [nwin][nxl + 2]
    const T *hlines;           // the halo lines HL[nwin + 1][nxl + 2][32] (step_march3.hpp), levels 0 .. depth-1 of every (seam, column)
    T *seams;                  // S3[nwin + 1][nxl + 2][M3_SREC]: the rows around every window seam of the DESTINATION lattice (step_march3.hpp)
    const MarchUnit *units;
    int nunits;
    Geom g;
    unsigned lat_bytes;        // bytes of one lattice (9 planes) — below 4 GiB
    int nwin_total;            // windows per column
    int win_stride = 0;        // k_march3: rows from one window to the next (0: the window height, 64 S — windows that tile the column and take the rows
    int win_off = 0;           // beyond their seams out of the halo lines); OVERLAPPING windows (stride 64 S - 8, offset -4): see k_march3
    FastDiv fdv;               // fp32: tau and RN(1/tau)
    T tau;
    T U0;
    int rev;
    unsigned long long *clk = nullptr;   // tuning passes only (tune_fuse_plan): [unit] = {start, end} of every unit in s_memtime ticks
    unsigned int *stuck = nullptr;       // host-visible word: a chain unit that gave up waiting for its partner's hand-over sets it (step_chain.hpp)
};

// S consecutive rows of one column and direction, held by one lane
template <typename T, int S> struct MV { T v[S]; };
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
template <int BYTES> struct RawOf;
template <> struct RawOf<16> { typedef u4v type; };
template <> struct RawOf<8> { typedef u2v type; };

template <typename T, int S> __device__ __forceinline__ MV<T, S> mv_splat(T x)
{
    MV<T, S> r;
#pragma unroll
    for (int v = 0; v < S; v++) r.v[v] = x;
    return r;
}

// the value held by lane - 1 / lane + 1 as ONE data-parallel-primitive move each (v_mov_b32_dpp wave_shr:1 / wave_shl:1; lane 0 /
// lane 63 keep their own value) — __shfl_up / __shfl_down compile to ds_bpermute_b32, an LDS round trip with a wait behind it
__device__ __forceinline__ int dpp_wave_up(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int dpp_wave_down(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ float wave_up(float x) { return __int_as_float(dpp_wave_up(__float_as_int(x))); }
__device__ __forceinline__ float wave_down(float x) { return __int_as_float(dpp_wave_down(__float_as_int(x))); }
__device__ __forceinline__ double wave_up(double x) { return __hiloint2double(dpp_wave_up(__double2hiint(x)), dpp_wave_up(__double2loint(x))); }
__device__ __forceinline__ double wave_down(double x) { return __hiloint2double(dpp_wave_down(__double2hiint(x)), dpp_wave_down(__double2loint(x))); }

// The values at rows j-1 / j+1 of a lane's sites (shifted by one lane), the row outside the window taken straight out of the column's halo register `hv` (step_march3.hpp: lanes 0..15 hold the words that
// come from below, lanes 48..63 those from above) by a ROW shift — lane N into lane 0 (resp. lane 48 + P into lane 63) — and the wave shift then leaving
// that lane alone: two data-parallel-primitive moves per direction instead of a v_readlane, a move and a select (the kernel is bound by the number of
// vector instructions it issues, and the six wave-uniform edge values of every stage no longer pass through scalar registers).
template <int N> __device__ __forceinline__ int dpp_shift_below(int x, int hv)
{
    static_assert(N >= 0 && N < 16, "from-below words live in lanes 0..15");
    // (mov_dpp: the lanes the row shift does not write are don't-care — only lane 0 of `e` is used —, so the move needs no copy of hv in its destination first)
    int e = hv;
    if constexpr (N > 0) e = __builtin_amdgcn_mov_dpp(hv, 0x100 + N, 0x1, 0xf, false);               // row_shl:N, row 0 only: lane 0 <- lane N
    return __builtin_amdgcn_update_dpp(e, x, 0x138, 0xf, 0xf, false);                                   // wave_shr:1: lane i <- lane i-1, lane 0 keeps e
}
template <int P> __device__ __forceinline__ int dpp_shift_above(int x, int hv)
{
    static_assert(P >= 0 && P < 16, "from-above words live in lanes 48..63");
    int e = hv;
    if constexpr (P < 15) e = __builtin_amdgcn_mov_dpp(hv, 0x110 + (15 - P), 0x8, 0xf, false);          // row_shr:15-P, row 3 only: lane 63 <- lane 48+P
    return __builtin_amdgcn_update_dpp(e, x, 0x130, 0xf, 0xf, false);                                   // wave_shl:1: lane i <- lane i+1, lane 63 keeps e
}
template <int N> __device__ __forceinline__ float shift_below_h(float x, float hv) { return __int_as_float(dpp_shift_below<N>(__float_as_int(x), __float_as_int(hv))); }
template <int N> __device__ __forceinline__ double shift_below_h(double x, double hv)
{
    return __hiloint2double(dpp_shift_below<N>(__double2hiint(x), __double2hiint(hv)), dpp_shift_below<N>(__double2loint(x), __double2loint(hv)));
}
template <int P> __device__ __forceinline__ float shift_above_h(float x, float hv) { return __int_as_float(dpp_shift_above<P>(__float_as_int(x), __float_as_int(hv))); }
template <int P> __device__ __forceinline__ double shift_above_h(double x, double hv)
{
    return __hiloint2double(dpp_shift_above<P>(__double2hiint(x), __double2hiint(hv)), dpp_shift_above<P>(__double2loint(x), __double2loint(hv)));
}
template <int N, typename T, int S> __device__ __forceinline__ MV<T, S> m_below_h(const MV<T, S> &r, T hv)
{
    MV<T, S> o;
    o.v[0] = shift_below_h<N>(r.v[S - 1], hv);
#pragma unroll
    for (int v = 1; v < S; v++) o.v[v] = r.v[v - 1];
    return o;
}
template <int P, typename T, int S> __device__ __forceinline__ MV<T, S> m_above_h(const MV<T, S> &r, T hv)
{
    MV<T, S> o;
#pragma unroll
    for (int v = 0; v < S - 1; v++) o.v[v] = r.v[v + 1];
    o.v[S - 1] = shift_above_h<P>(r.v[0], hv);
    return o;
}
// ... and for OVERLAPPING windows (OVL; k_march3): the first / last lane's row beyond the window is a margin row's input — don't-care —, so the wave
// shift alone (that lane keeps its own value: finite) does, one data-parallel-primitive move per direction
template <int N, bool OVL, typename T, int S> __device__ __forceinline__ MV<T, S> m_below_x(const MV<T, S> &r, T hv)
{
    if constexpr (!OVL) return m_below_h<N>(r, hv);
    else {
        MV<T, S> o;
        o.v[0] = wave_up(r.v[S - 1]);
#pragma unroll
        for (int v = 1; v < S; v++) o.v[v] = r.v[v - 1];
        return o;
    }
}
template <int P, bool OVL, typename T, int S> __device__ __forceinline__ MV<T, S> m_above_x(const MV<T, S> &r, T hv)
{
    if constexpr (!OVL) return m_above_h<P>(r, hv);
    else {
        MV<T, S> o;
#pragma unroll
        for (int v = 0; v < S - 1; v++) o.v[v] = r.v[v + 1];
        o.v[S - 1] = wave_down(r.v[0]);
        return o;
    }
}

// buffer addressing: rsrc = whole lattice; voff = the lane's byte offset (j0 * sizeof(T), loop-invariant);
// soff = scalar byte offset of (plane, column, row shift)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t march_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
template <typename T, int S>
__device__ __forceinline__ MV<T, S> bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    MV<T, S> o;
    if constexpr (S * sizeof(T) == 16) {
        const u4v x = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, WT_LOAD_AUX);
        __builtin_memcpy(&o, &x, 16);
    } else {
        const u2v x = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, WT_LOAD_AUX);
        __builtin_memcpy(&o, &x, 8);
    }
    return o;
}
template <typename T, int S>
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const MV<T, S> &v)
{
    typename RawOf<S * sizeof(T)>::type x;
    __builtin_memcpy(&x, &v, S * sizeof(T));
    if constexpr (S * sizeof(T) == 16) __builtin_amdgcn_raw_buffer_store_b128(x, r, voff, soff, WT_STORE_AUX);
    else __builtin_amdgcn_raw_buffer_store_b64(x, r, voff, soff, WT_STORE_AUX);
}
// STORE-DATA HAZARD (measured on MI355X, ROCm 7.2): a buffer_store_dwordx4 whose soffset is an SGPR reads its data
// VGPRs a little after it issues.  A VALU instruction right behind it that overwrites one of them can win that race for
// the last lanes of each 16-lane group when the memory pipe is backed up — the store then writes the NEW register
// contents (seen as 4-lane groups of wrong macro values at the outlet column of a 16384 x 4096 lattice, nowhere else
// and not on every run).  hipcc pads this hazard only for stores WITHOUT a register soffset (LLVM GCNHazardRecognizer::
// createsVALUHazard), so the pad is ours: the asm keeps the data tuples of a pair of 16-byte stores (the seam records,
// step_march3.hpp seam3_flush) live up to this point and its `s_nop 1` gives the two wait states after the second.
// tools/check_store_hazard.py verifies the generated ISA (run by tests/test_build_hazards.py).  (8-byte stores — the
// lattice's — have no such hazard; the fence is empty for them.)
template <typename R>
__device__ __forceinline__ void store_data_fence2(const R &a, const R &b)
{
    if constexpr (sizeof(R) == 16) asm volatile("s_nop 1" ::"v"(a), "v"(b));
}

template <typename T, int S>
struct MarchAddr {
    __amdgpu_buffer_rsrc_t rs, rd, rm;   // source lattice, destination lattice, macro planes
    unsigned voff;                       // j0 * sizeof(T)
    unsigned voff_st;                    // the same for stores; lanes beyond the last row: out of range (dropped by the buffer check)
    int lane;
    unsigned P4, pitch4, mp4;            // plane / column / macro-plane strides in bytes
    char *own_lds;                       // k_march3, general (BODY) units: this wave's two LDS buffers for a column's own populations (own_prefetch); else null
    unsigned voff_dma;                   // the lane's byte offset for a dword-per-lane LDS-DMA load of the window's first 64 dwords: row0 * sizeof(T) + 4 lane
};

// byte offset of (plane k, local column col, row shift dj) from the lattice base (one pad column in front)
template <typename T, int S>
__device__ __forceinline__ unsigned lat_off(const MarchAddr<T, S> &a, int k, int col, int dj)
{
    return (unsigned)k * a.P4 + (unsigned)(col + 1) * a.pitch4 + (unsigned)(dj * (int)sizeof(T));
}

// The nine streamed (pulled) input vectors of column `col`, loaded WITHOUT the row shift: every load is the window's own 64 S rows of the upstream column — 4 whole 128-byte
// lines (fp32) instead of 5, the fifth being a line of the neighbouring window that its wave fetches as well.  The shift by one row happens
// in registers (march_align_in), the row outside the window comes from the column's halo line (level-0 words, step_march3.hpp).
// Measured before: 46.7 line requests per column and window against 36 + 1 (profiles/r04_u_fetch_calibration.txt).
template <typename T, int S>
__device__ __forceinline__ void march_load_aligned(const MarchAddr<T, S> &a, int col, MV<T, S> (&fin)[9])
{
    fin[0] = bload<T, S>(a.rs, a.voff, lat_off(a, 0, col, 0));
    fin[1] = bload<T, S>(a.rs, a.voff, lat_off(a, 1, col - 1, 0));
    fin[3] = bload<T, S>(a.rs, a.voff, lat_off(a, 3, col + 1, 0));
    fin[2] = bload<T, S>(a.rs, a.voff, lat_off(a, 2, col, 0));
    fin[5] = bload<T, S>(a.rs, a.voff, lat_off(a, 5, col - 1, 0));
    fin[6] = bload<T, S>(a.rs, a.voff, lat_off(a, 6, col + 1, 0));
    fin[4] = bload<T, S>(a.rs, a.voff, lat_off(a, 4, col, 0));
    fin[7] = bload<T, S>(a.rs, a.voff, lat_off(a, 7, col + 1, 0));
    fin[8] = bload<T, S>(a.rs, a.voff, lat_off(a, 8, col - 1, 0));
}

// S mask / bounce-code bytes of a lane's sites, site v in bits 8v .. 8v+7
template <int S> __device__ __forceinline__ uint32_t load_site_bytes(const uint8_t *p)
{
    if constexpr (S == 4) return *reinterpret_cast<const uint32_t *>(p);
    else if constexpr (S == 2) return *reinterpret_cast<const uint16_t *>(p);
    else return *p;
}

// The solid flags and bounce codes of a lane's sites in one column do not depend on the level, and a unit's general loop needs them for
// the same column at consecutive iterations (STEP_FS at x, the next level at x - 1, ...).  Fetched inside the stage that uses them they
// sit behind a scalar branch, and hipcc's wait for them drains vmcnt to 0 — the prefetched column and the stores of the previous
// iteration included: a round trip to memory per level and iteration (27 such waits in the four-step general loop; per-unit clocks: a body
// column cost 3.2 plain ones).  Fetched ONE ITERATION AHEAD for every column of a general unit, beside the prefetched populations, and
// handed down from level to level in registers, they cost two byte loads per iteration and no wait of their own.
struct SiteBytes { uint32_t v[2]; };     // {solid4, code4}
// the row a lane's mask / bounce-code bytes are fetched from: its own first row, or — the margin lanes of an overlapping window below row 0 or beyond
// the last row (k_march3), whose results nobody stores — the nearest rows that exist
template <int S, bool OVL> __device__ __forceinline__ int site_row(int j0, int ny)
{
    if constexpr (OVL) return j0 < 0 ? 0 : (j0 > ny - S ? ny - S : j0);
    else return j0;
}
template <typename T, int S, bool OVL = false>
__device__ __forceinline__ SiteBytes site_bytes_load(const MarchParams<T> &p, int col, int j0)
{
    const int c = col < 0 ? 0 : (col > p.g.nxl - 1 ? p.g.nxl - 1 : col);       // (columns outside carry no class: their bytes are never used)
    const int jb = site_row<S, OVL>(j0, p.g.ny);
    SiteBytes r;
    r.v[0] = load_site_bytes<S>(p.mask + (long)(c + 1) * p.g.pitch + jb);
    r.v[1] = load_site_bytes<S>(p.bcode + (long)c * p.g.pitch + jb);
    return r;
}

// Two fp32 sites per lane as 2-vectors: the operations of collide_head / collide_tail (d2q9.hpp), element for element, written
// on float2 so that hipcc emits packed instructions (v_pk_add / v_pk_mul / v_pk_fma_f32) without the register-shuffling moves
// its SLP vectoriser pays for the same pairs (a third of the loop's vector instructions go away).  Selected by bit 2 of FD
// (MARCH_FD_PACKED): measured in alternating runs on one box it gains 3.4 % in the four-step kernel (158 -> 163 GLUPS), which
// is bound by its instruction stream, and loses 1-1.5 % in the three-step kernel on slab-sized lattices.
static constexpr int MARCH_FD_PACKED = 4;
// bit 6 of FD, set beside MARCH_FD_PACKED by the four-step kernel's NON-EMITTING instantiations (step_chain.hpp k_march3): the plain columns' collision
// shares one reciprocal between the two velocity divisions (collide2_shared below).  The emitting ones — one pass per readout — stand at 255 of 256
// registers as they are, and the decision's two momenta would spill there.
static constexpr int MARCH_FD_VELSHARED = 64;
typedef float f2v __attribute__((ext_vector_type(2)));
// a / b for two sites at once, operation for operation hipcc's own expansion of the IEEE binary32 division (LLVM AMDGPUTargetLowering::LowerFDIV32 with
// fp32 denormals on: v_div_scale x2, v_rcp, fma, fma, mul, fma, fma, fma, v_div_fmas, v_div_fixup) — the same instructions on the same values, so the same
// bits — with the six multiply-adds in between as PACKED instructions over the two sites: the marching kernel is bound by the number of vector
// instructions it issues (an un-packed collision costs it 20 %), and the two divisions per site were a sixth of them.
__device__ __forceinline__ f2v div2_ieee(f2v a, f2v b)
{
    bool s0, s1, dummy;
    const f2v ds = {__builtin_amdgcn_div_scalef(a[0], b[0], false, &dummy), __builtin_amdgcn_div_scalef(a[1], b[1], false, &dummy)};     // denominator scaled
    const f2v ns = {__builtin_amdgcn_div_scalef(a[0], b[0], true, &s0), __builtin_amdgcn_div_scalef(a[1], b[1], true, &s1)};             // numerator scaled
    const f2v rc = {__builtin_amdgcn_rcpf(ds[0]), __builtin_amdgcn_rcpf(ds[1])};
    const f2v one = {1.0f, 1.0f};
    const f2v f0 = __builtin_elementwise_fma(-ds, rc, one);
    const f2v f1 = __builtin_elementwise_fma(f0, rc, rc);
    const f2v mu = ns * f1;
    const f2v f2 = __builtin_elementwise_fma(-ds, mu, ns);
    const f2v f3 = __builtin_elementwise_fma(f2, f1, mu);
    const f2v f4 = __builtin_elementwise_fma(-ds, f3, ns);
    f2v q;
    q[0] = __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(f4[0], f1[0], f3[0], s0), b[0], a[0]);
    q[1] = __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(f4[1], f1[1], f3[1], s1), b[1], a[1]);
    return q;
}

// nu / rs and nv / rs for two sites on ONE reciprocal per site: the operations of div2_ieee without its v_div_scale, v_div_fmas and v_div_fixup, the
// reciprocal and its two refinements — which see the denominator alone — computed once for both numerators.  The same bits as two div2_ieee calls
// wherever veldiv_guard (below) holds; operand by operand, from the definitions of the three instructions (b = rs the denominator, a a numerator):
//   v_div_scale_f32 returns its operand unchanged and clears VCC unless one of these holds, tested in this order: a or b is zero (NaN: see +0 below);
//     exponent(a) - exponent(b) >= 96 (here a < 12, b >= 0.5: at most 4); b subnormal (b >= 0.5); 1 / b subnormal (b < 18); a / b subnormal
//     (|a| >= 2^-103, b < 18: |a / b| > 2^-108); biased exponent of a <= 23, i.e. |a| < 2^-103 (excluded).  So ds = b, ns = a, and rc, f0 .. f4 below are
//     div2_ieee's values.
//   v_div_fmas_f32 is fma(f4, f1, f3), times 2^32 only where VCC is set: here the plain fma.
//   v_div_fixup_f32(q, b, a) returns q with the sign of a / b for finite non-zero a and b unless exponent(a) - exponent(b) is below -150 or the
//     exponent of b is 255 (neither here); q is within an ulp of a / b, of magnitude above 2^-108, hence non-zero, normal and of that sign already.
//   a = +0: v_div_fixup_f32 returns (sign a xor sign b) 0 = +0 whatever the NaN chain before it computed; here mu = +0 f1 = +0 (f1 > 0), f2 = fma(-b, +0, +0)
//     = -0 + +0 = +0, f3 = fma(+0, f1, +0) = +0, f4 = +0, q = +0.  (a = -0 would give +0 as well where the division gives -0: the guard keeps it out.)
// tools/veldiv_check.c runs the chain on the CPU with every float within one ulp of 1 / b in place of v_rcp_f32's against the correctly rounded quotient;
// k_check_veldiv below compares it with the division on the device.
__device__ __forceinline__ void div2_shared(f2v nu, f2v nv, f2v rs, f2v &u, f2v &v)
{
    const f2v rc = {__builtin_amdgcn_rcpf(rs[0]), __builtin_amdgcn_rcpf(rs[1])};
    const f2v one = {1.0f, 1.0f};
    const f2v f0 = __builtin_elementwise_fma(-rs, rc, one);
    const f2v f1 = __builtin_elementwise_fma(f0, rc, rc);
    const f2v mu = nu * f1, mv = nv * f1;
    const f2v f2u = __builtin_elementwise_fma(-rs, mu, nu), f2w = __builtin_elementwise_fma(-rs, mv, nv);
    const f2v f3u = __builtin_elementwise_fma(f2u, f1, mu), f3v = __builtin_elementwise_fma(f2w, f1, mv);
    const f2v f4u = __builtin_elementwise_fma(-rs, f3u, nu), f4v = __builtin_elementwise_fma(-rs, f3v, nv);
    u = __builtin_elementwise_fma(f4u, f1, f3u);
    v = __builtin_elementwise_fma(f4v, f1, f3v);
}

// Pair number i of the self-test's stream (tools/veldiv_check.c builds the same on the CPU), inside the ranges veldiv_guard admits.  Even i, pseudo-random:
// b uniform in significand over the binades of [0.5, 18), a over the binades of [2^-103, 12), either sign.  Odd i, built: a = +0; a and b a few ulps inside
// either end of their ranges; else a = RN(m b) -3 .. +3 ulps for the midpoint m above a float q (as k_check_fastdiv64 builds them), q in [2^-101, 2^-1).
__device__ __forceinline__ void veldiv_pair(unsigned long long seed, unsigned long long i, float &a, float &b)
{
    auto mix = [](unsigned long long z) { z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); };
    constexpr unsigned A_MIN = 0x0c000000u, A_END = 0x41400000u, B_MIN = 0x3f000000u, B_END = 0x41900000u;      // 2^-103, 12, 0.5, 18
    const unsigned long long z = mix(seed + 0x9e3779b97f4a7c15ULL * (i + 1)), y = mix(z);
    const unsigned eb = 126u + (unsigned)((z >> 23) % 6u);
    unsigned bb = (eb << 23) | (unsigned)(z & 0x7fffffu);
    if (bb >= B_END) bb = (eb << 23) | (unsigned)(z & 0xfffffu);
    const unsigned sign = (unsigned)(z >> 63) << 31;
    unsigned ab;
    if (!(i & 1)) {
        const unsigned ea = 24u + (unsigned)((z >> 32) % 107u);
        ab = (ea << 23) | (unsigned)(y & 0x7fffffu);
        if (ab >= A_END) ab = (ea << 23) | (unsigned)(y & 0x3fffffu);
        ab |= sign;
    } else if ((i & 14) == 2) {
        ab = 0;
    } else if ((i & 14) == 4) {
        const unsigned da = (unsigned)(y & 7u), db = (unsigned)((y >> 3) & 7u);
        ab = (((y >> 6) & 1u) ? A_END - 1u - da : A_MIN + da) | sign;
        bb = ((y >> 7) & 1u) ? B_END - 1u - db : B_MIN + db;
    } else {
        const unsigned eq = (unsigned)(26u + (z >> 32) % 100u) << 23;
        const float q = __uint_as_float(eq | (unsigned)(y & 0x7fffffu)), bf = __uint_as_float(bb);
        const float xm = __builtin_fmaf(q, bf, (__uint_as_float(eq) * 0x1p-24f) * bf);       // (2^e 2^-24: half an ulp of q; times b: exact)
        ab = (__float_as_uint(xm) + (unsigned)((y >> 60) & 7u) - 3u) | sign;
    }
    a = __uint_as_float(ab);
    b = __uint_as_float(bb);
}
// option "selftest_veldiv": mismatches of div2_shared against the division, 4 n pairs per thread (tests/test_gpu_veldiv.py)
__global__ void k_check_veldiv(unsigned long long seed, int n, unsigned int *__restrict__ nbad)
{
    const unsigned long long t = (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x);
    unsigned int bad = 0;
    for (int it = 0; it < n; it++) {
        float a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) veldiv_pair(seed, (t * (unsigned long long)n + (unsigned long long)it) * 4ULL + (unsigned long long)j, a[j], b[j]);
        // two sites: denominators b[0], b[1] (those of pairs 2, 3 go unused), numerators a[0], a[1] and a[2], a[3]
        f2v u, v;
        div2_shared(f2v{a[0], a[1]}, f2v{a[2], a[3]}, f2v{b[0], b[1]}, u, v);
        bad += (__float_as_uint(u[0]) != __float_as_uint(a[0] / b[0])) + (__float_as_uint(u[1]) != __float_as_uint(a[1] / b[1]));
        bad += (__float_as_uint(v[0]) != __float_as_uint(a[2] / b[0])) + (__float_as_uint(v[1]) != __float_as_uint(a[3] / b[1]));
    }
    if (bad) atomicAdd(nbad, bad);
}

// This lane's two sites may take div2_shared, the one-sided density clamp and the fast division by tau.  Decided before the velocities exist, on the raw
// bits, as unsigned integers (a non-negative float orders like its bits; a set sign bit or a NaN lies above every finite non-negative one):
//   every population in [+0, 2): no NaN, no infinity, nothing negative and no -0; so 0 <= rho < 18, the momenta are finite and below 12 in magnitude, and
//     no momentum is -0 — a sum of six terms is -0 only if every term is, which takes fin[1] (fin[2]) = -0;
//   rho >= 0.5 (so the lower density clamp does nothing);
//   each of the four momenta +0 or of magnitude >= 2^-103: (bits << 1) - 1 puts +0 on top and orders the rest by magnitude.
__device__ __forceinline__ bool veldiv_guard(const f2v (&fin)[9], f2v rs, f2v nu, f2v nv)
{
    auto bits = [](float x) { return __builtin_bit_cast(unsigned, x); };
    auto max3 = [](unsigned a, unsigned b, unsigned c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); };
    auto mag = [&](float x) { return (bits(x) << 1) - 1u; };
    unsigned top[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
        top[i] = max3(max3(bits(fin[0][i]), bits(fin[1][i]), bits(fin[2][i])), max3(bits(fin[3][i]), bits(fin[4][i]), bits(fin[5][i])),
                      max3(bits(fin[6][i]), bits(fin[7][i]), bits(fin[8][i])));
    const unsigned a = mag(nu[0]), b = mag(nu[1]), c = mag(nv[0]), d = mag(nv[1]);
    const unsigned low3 = a < b ? (a < c ? a : c) : (b < c ? b : c), low = low3 < d ? low3 : d;
    return top[0] < 0x40000000u && top[1] < 0x40000000u && rs[0] >= 0.5f && rs[1] >= 0.5f && low >= 2u * 0x0c000000u - 1u;
}

// fo = fin - (fin - eq) / tau for two sites, the division in two / three operations (d2q9.hpp div_by_tau_fast)
template <bool TWO_OP>
__device__ __forceinline__ void relax2_fast(const f2v (&fin)[9], const f2v (&eq)[9], const FastDiv &fdv, f2v (&fo)[9])
{
    const f2v rt = {fdv.rtau, fdv.rtau}, ta = {fdv.tau, fdv.tau}, rl = {fdv.rlo, fdv.rlo};
    // three directions abreast: a packed fp32 instruction whose result the very next instruction needs costs a wait state (s_nop) —
    // written chain by chain the nine relaxations were a fifth of the loop's issue slots in nops
#pragma unroll
    for (int g = 0; g < 9; g += 3) {
        f2v x[3], q0[3], e[3], t[3];
#pragma unroll
        for (int j = 0; j < 3; j++) x[j] = fin[g + j] - eq[g + j];
        if constexpr (TWO_OP) {      // div_by_tau_fast<true>: p = x rlo, q = fma(x, r, p)
#pragma unroll
            for (int j = 0; j < 3; j++) q0[j] = x[j] * rl;
#pragma unroll
            for (int j = 0; j < 3; j++) t[j] = __builtin_elementwise_fma(x[j], rt, q0[j]);
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++) q0[j] = x[j] * rt;
#pragma unroll
            for (int j = 0; j < 3; j++) e[j] = __builtin_elementwise_fma(-q0[j], ta, x[j]);
#pragma unroll
            for (int j = 0; j < 3; j++) t[j] = __builtin_elementwise_fma(e[j], rt, q0[j]);
        }
#pragma unroll
        for (int j = 0; j < 3; j++) fo[g + j] = fin[g + j] - t[j];
    }
}

template <int FD, bool TWO_OP>
__device__ __forceinline__ void collide2_packed(const f2v (&fin)[9], const FastDiv &fdv, f2v (&fo)[9], f2v &rho, f2v &ux, f2v &uy)
{
    f2v r, u, v;
    {   // moments (d2q9.hpp, html:335-338) with the two divisions packed
        // (0.0 + fin[0] of the reference's sum is fin[0] itself unless fin[0] = -0, and a density sum that starts at -0 instead of +0 ends on the same
        //  value unless all nine populations are -0 — a state whose clamped density, 0.5, and NaN velocity are the same either way: the addition is dropped)
        f2v rs = fin[0];
#pragma unroll
        for (int k = 1; k < 9; k++) rs += fin[k];
        r = rs;
        u = div2_ieee(fin[1] + fin[5] + fin[8] - fin[3] - fin[6] - fin[7], rs);
        v = div2_ieee(fin[2] + fin[5] + fin[6] - fin[4] - fin[7] - fin[8], rs);
    }
    const float rhoMin = 0.5f, rhoMax = 2.0f, uMax = 0.35f;        // html:344
#pragma unroll
    for (int i = 0; i < 2; i++) {
        float ri = r[i];
        ri = (ri < rhoMin) ? rhoMin : ri;
        ri = (rhoMax < ri) ? rhoMax : ri;
        r[i] = ri;
    }
    const f2v spd2 = u * u + v * v;
    bool safe = true;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const float m0 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(fin[0][i]), __builtin_fabsf(fin[1][i])), __builtin_fabsf(fin[2][i]));
        const float m1 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(fin[3][i]), __builtin_fabsf(fin[4][i])), __builtin_fabsf(fin[5][i]));
        const float m2 = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(fin[6][i]), __builtin_fabsf(fin[7][i])), __builtin_fabsf(fin[8][i]));
        const float m = __builtin_fmaxf(__builtin_fmaxf(m0, m1), m2);
        safe = safe && (m < 0x1p100f) && (r[i] == r[i]) && (spd2[i] == spd2[i]);
    }
    const bool fast = (FD == 2) || (FD == 1 && __ballot(!safe) == 0ULL);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        if (spd2[i] > uMax * uMax) {
            const float k = uMax / wt_sqrt<float>(spd2[i]);
            u[i] *= k;
            v[i] *= k;
        }
    }
    f2v eq[9];
    feq_all<f2v>(r, u, v, eq);
    if (FD != 0 && fast) {
        relax2_fast<TWO_OP>(fin, eq, fdv, fo);
    } else {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const f2v x = fin[k] - eq[k];
            f2v q;
            q[0] = x[0] / fdv.tau; q[1] = x[1] / fdv.tau;
            fo[k] = fin[k] - q;
        }
    }
    rho = r; ux = u; uy = v;
}

// collide2_packed for the plain columns, with ONE wave-uniform decision per collision, taken before the velocities exist: every lane's two sites in the
// ranges of veldiv_guard — div2_shared, the upper density clamp alone, the fast division by tau —, or the whole wave through collide2_packed as it stands.
// The same bits either way (div2_shared, d2q9.hpp): the decision is a matter of speed alone.  FD = 1 only; the general (body) columns keep
// collide2_packed: their loop holds every input population across the collision and stands at 255 of 256 registers without the two momenta.
template <bool TWO_OP>
__device__ __forceinline__ void collide2_shared(const f2v (&fin)[9], const FastDiv &fdv, f2v (&fo)[9], f2v &rho, f2v &ux, f2v &uy)
{
    f2v rs = fin[0];                     // (as collide2_packed)
#pragma unroll
    for (int k = 1; k < 9; k++) rs += fin[k];
    const f2v nu = fin[1] + fin[5] + fin[8] - fin[3] - fin[6] - fin[7], nv = fin[2] + fin[5] + fin[6] - fin[4] - fin[7] - fin[8];
    unsigned long long out = __ballot(!veldiv_guard(fin, rs, nu, nv));       // lanes with a site outside the guard's ranges
    asm("" : "+s"(out));                 // a scalar compare and branch on the mask itself (hipcc otherwise branches on VCC, the rare path laid out first)
    if (__builtin_expect(out == 0ULL, 1)) {
        const float rhoMax = 2.0f, uMax = 0.35f;                   // html:344
        f2v r, u, v;
        div2_shared(nu, nv, rs, u, v);
        r[0] = __builtin_fminf(rs[0], rhoMax); r[1] = __builtin_fminf(rs[1], rhoMax);           // (0.5 <= rho, no NaN: the clamp's upper half is all of it)
        const f2v spd2 = u * u + v * v;                                                          // (finite: |u|, |v| < 24)
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (spd2[i] > uMax * uMax) {
                const float k = uMax / wt_sqrt<float>(spd2[i]);
                u[i] *= k;
                v[i] *= k;
            }
        }
        f2v eq[9];
        feq_all<f2v>(r, u, v, eq);
        relax2_fast<TWO_OP>(fin, eq, fdv, fo);
        rho = r; ux = u; uy = v;
    } else collide2_packed<1, TWO_OP>(fin, fdv, fo, rho, ux, uy);
}

// collide S sites per lane; fp32: one wave-uniform decision between the fast and the IEEE division by tau — and, VEL_SHARED (MARCH_FD_VELSHARED on a plain
// column, with a proved division by tau), the velocity divisions: collide2_shared
template <typename T, int S, int FD, bool VEL_SHARED = false>
__device__ __forceinline__ void march_collide_sites(const MV<T, S> (&fin)[9], const FastDiv &fdv, T tau, MV<T, S> (&o)[9], MV<T, S> &rho4, MV<T, S> &ux4,
                                                    MV<T, S> &uy4)
{
    constexpr int FDV = FD & 3;          // how to divide by tau (d2q9.hpp)
    constexpr bool TWO = (FD & MARCH_FD_TWOOP) != 0;
    if constexpr (sizeof(T) == 4 && (FD & MARCH_FD_CONTRACTED) != 0) {
#pragma unroll
        for (int v = 0; v < S; v++) {
            float a[9], f[9], r, u, w;
#pragma unroll
            for (int k = 0; k < 9; k++) a[k] = fin[k].v[v];
            collide_contracted(a, fdv.rtau, f, r, u, w);
#pragma unroll
            for (int k = 0; k < 9; k++) o[k].v[v] = f[k];
            rho4.v[v] = r; ux4.v[v] = u; uy4.v[v] = w;
        }
    } else if constexpr (sizeof(T) == 4 && S == 2 && (FD & MARCH_FD_PACKED) != 0) {
        f2v a[9], f[9], r, u, w;
#pragma unroll
        for (int k = 0; k < 9; k++) a[k] = f2v{fin[k].v[0], fin[k].v[1]};
        if constexpr (VEL_SHARED && FDV == 1) collide2_shared<TWO>(a, fdv, f, r, u, w);
        else collide2_packed<FDV, TWO>(a, fdv, f, r, u, w);
#pragma unroll
        for (int k = 0; k < 9; k++) { o[k].v[0] = f[k][0]; o[k].v[1] = f[k][1]; }
        rho4.v[0] = r[0]; rho4.v[1] = r[1]; ux4.v[0] = u[0]; ux4.v[1] = u[1]; uy4.v[0] = w[0]; uy4.v[1] = w[1];
    } else if constexpr (sizeof(T) == 4) {
        float r[S], u[S], w[S], s2[S];
        bool safe = true;
#pragma unroll
        for (int v = 0; v < S; v++) {
            float a[9];
            bool sv;
#pragma unroll
            for (int k = 0; k < 9; k++) a[k] = fin[k].v[v];
            collide_head(a, r[v], u[v], w[v], s2[v], sv);
            safe = safe && sv;
        }
        const bool fast = (FDV == 2) || (FDV == 1 && __ballot(!safe) == 0ULL);
#pragma unroll
        for (int v = 0; v < S; v++) {
            float a[9], f[9];
#pragma unroll
            for (int k = 0; k < 9; k++) a[k] = fin[k].v[v];
            if (FDV != 0 && fast) collide_tail<true, TWO>(a, fdv, r[v], u[v], w[v], s2[v], f);
            else collide_tail<false>(a, fdv, r[v], u[v], w[v], s2[v], f);
#pragma unroll
            for (int k = 0; k < 9; k++) o[k].v[v] = f[k];
            rho4.v[v] = r[v]; ux4.v[v] = u[v]; uy4.v[v] = w[v];
        }
    } else {
#pragma unroll
        for (int v = 0; v < S; v++) {
            T a[9], f[9], r, u, w;
#pragma unroll
            for (int k = 0; k < 9; k++) a[k] = fin[k].v[v];
            collide_t<T, FD>(a, fdv, tau, f, r, u, w);
#pragma unroll
            for (int k = 0; k < 9; k++) o[k].v[v] = f[k];
            rho4.v[v] = r; ux4.v[v] = u; uy4.v[v] = w;
        }
    }
}

template <typename T, int S, int FD, bool WANT_MACRO>
__device__ __forceinline__ void march_collide(const MV<T, S> (&fin)[9], const FastDiv &fdv, T tau, MV<T, S> (&G)[9], MV<T, S> (&mac)[3])
{
    MV<T, S> rho4, ux4, uy4;
    march_collide_sites<T, S, FD, (FD & MARCH_FD_VELSHARED) != 0>(fin, fdv, tau, G, rho4, ux4, uy4);
    if (WANT_MACRO) { mac[0] = rho4; mac[1] = ux4; mac[2] = uy4; }
}

// rows 0 and NY-1 carry the far-field populations (html:314-322); only called for windows that hold one of them
template <typename T, int S, bool WANT_MACRO>
__device__ __forceinline__ void march_far_rows(int j0, int ny, T U0, const T (&feq0)[9], MV<T, S> (&G)[9], MV<T, S> (&mac)[3])
{
#pragma unroll
    for (int v = 0; v < S; v++) {
        const int j = j0 + v;
        const bool far = (j == 0) || (j == ny - 1);
#pragma unroll
        for (int k = 0; k < 9; k++) G[k].v[v] = far ? feq0[k] : G[k].v[v];
        if (WANT_MACRO) { mac[0].v[v] = far ? T(1) : mac[0].v[v]; mac[1].v[v] = far ? U0 : mac[1].v[v]; mac[2].v[v] = far ? T(0) : mac[2].v[v]; }
    }
}

// GENERAL tile, before the collision: half-way bounce-back (html:324-334) as an in-place select —
// direction k of a site takes the site's OWN population opp(k) where the bounce code has bit k-1 set.
// `own(k)` yields the vector of the sites' own populations of direction k (step 1: an aligned load,
// step 2: the step-1 vector of column c held in registers); one vector is live at a time.
template <typename T, int S, typename OWN>
__device__ __forceinline__ void march_bounce(MV<T, S> (&fin)[9], uint32_t code4, OWN own)
{
#pragma unroll
    for (int k = 1; k < 9; k++) {
        const MV<T, S> o = own(opp_of(k));
#pragma unroll
        for (int v = 0; v < S; v++) fin[k].v[v] = ((code4 >> (8 * v + k - 1)) & 1u) ? o.v[v] : fin[k].v[v];
    }
}

// GENERAL tile, the collision itself.  `fin` went through march_bounce with code 0xFF on solid sites, i.e. a solid
// site's fin[k] already IS its own population opp(k) — the value the reference stores for it (html:287-294) — so the
// solid select needs no further loads.  Reference order: solid, far field (html:314-322), interior (html:335-359).
template <typename T, int S, int FD, bool WANT_MACRO>
__device__ __forceinline__ void march_collide_general(const MV<T, S> (&fin)[9], uint32_t solid4, int j0, int ny, const FastDiv &fdv, T tau, T U0,
                                                      const T (&feq0)[9], MV<T, S> (&G)[9], MV<T, S> (&mac)[3])
{
    MV<T, S> o[9], rho4, ux4, uy4;
    march_collide_sites<T, S, FD>(fin, fdv, tau, o, rho4, ux4, uy4);
#pragma unroll
    for (int v = 0; v < S; v++) {
        const bool solid = ((solid4 >> (8 * v)) & 0xffu) != 0;
        const int j = j0 + v;
        const bool far = (j == 0) || (j == ny - 1);
#pragma unroll
        for (int k = 0; k < 9; k++) G[k].v[v] = solid ? fin[k].v[v] : (far ? feq0[k] : o[k].v[v]);
        if (WANT_MACRO) {
            mac[0].v[v] = (solid || far) ? T(1) : rho4.v[v];
            mac[1].v[v] = solid ? T(0) : (far ? U0 : ux4.v[v]);
            mac[2].v[v] = (solid || far) ? T(0) : uy4.v[v];
        }
    }
}

// after the collision: solid sites carry their own populations reversed (html:287-294), macro (1,0,0)
template <typename T, int S, bool WANT_MACRO, typename OWN>
__device__ __forceinline__ void march_solid(MV<T, S> (&G)[9], MV<T, S> (&mac)[3], uint32_t solid4, OWN own)
{
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const MV<T, S> o = own(opp_of(k));
#pragma unroll
        for (int v = 0; v < S; v++) G[k].v[v] = ((solid4 >> (8 * v)) & 0xffu) ? o.v[v] : G[k].v[v];
    }
    if (WANT_MACRO) {
#pragma unroll
        for (int v = 0; v < S; v++) {
            const bool solid = ((solid4 >> (8 * v)) & 0xffu) != 0;
            mac[0].v[v] = solid ? T(1) : mac[0].v[v]; mac[1].v[v] = solid ? T(0) : mac[1].v[v]; mac[2].v[v] = solid ? T(0) : mac[2].v[v];
        }
    }
}

// outlet column (html:301-312): macro = moments of the copied populations, not clamped
template <typename T, int S>
__device__ __forceinline__ void march_outlet_macro(const MV<T, S> (&q9)[9], MV<T, S> (&mac)[3])
{
#pragma unroll
    for (int v = 0; v < S; v++) {
        T q[9], rho, ux, uy;
#pragma unroll
        for (int k = 0; k < 9; k++) q[k] = q9[k].v[v];
        moments(q, rho, ux, uy);
        mac[0].v[v] = rho; mac[1].v[v] = ux; mac[2].v[v] = uy;
    }
}

// march_load_aligned's inputs of one column -> the streamed (pulled) inputs: populations 2,5,6 come from one row below, 4,7,8 from one row above;
// `hv` = the column's halo words, level 0 in lanes 12..14 (from below) and 60..62 (from above)
template <bool OVL = false, typename T, int S>
__device__ __forceinline__ void march_align_in(MV<T, S> (&in)[9], int lane, T hv)
{
    in[2] = m_below_x<12, OVL>(in[2], hv); in[5] = m_below_x<13, OVL>(in[5], hv); in[6] = m_below_x<14, OVL>(in[6], hv);
    in[4] = m_above_x<12, OVL>(in[4], hv); in[7] = m_above_x<13, OVL>(in[7], hv); in[8] = m_above_x<14, OVL>(in[8], hv);
}
// a column's halo line — none for overlapping windows
template <bool OVL, typename T> __device__ __forceinline__ T halo_load_x(__amdgpu_buffer_rsrc_t rh, unsigned hoff, unsigned soff)
{
    if constexpr (OVL) return T(0);
    else if constexpr (sizeof(T) == 4) return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rh, hoff, soff, 0));
    else {
        const u2v x = __builtin_amdgcn_raw_buffer_load_b64(rh, hoff, soff, 0);
        return __hiloint2double((int)x.y, (int)x.x);
    }
}

// ---- a general column's OWN populations, prefetched into LDS (round 5) ----
// Step 1 of a column that touches the body needs the sites' own populations of all directions — the bounced values of half-way bounce-back
// (html:324-334: fin[k] = f[opp(k)] of the site itself where the upstream site is solid) and the reversed populations of solid sites
// (html:287-294).  Loaded where they are used they put a full trip to memory behind a scalar branch in the middle of an iteration: on the slab
// over the thick part of the body these nine loads ALONE were 20 % of the pass (profiles/r05_g_own_loads.txt: 21.1 -> 16.7 us per step with the
// loads stubbed out), and they are why a body column cost three plain ones.  There is no register to prefetch them into (242-253 VGPRs), so they
// go to LDS instead: at the top of the iteration BEFORE the one that needs them, ahead of that iteration's own prefetch, as dword-per-lane LDS-DMA
// loads (`buffer_load_dword ... lds`: lane i's dword lands at M0 + 4 i, so two instructions 256 bytes apart lay the window's 64 S sizeof(T) = 512
// bytes of one population down contiguously and every lane reads its S rows back with one ds_read_b64 — layout checked by tools/kldsdma.hip).
// Loads return in order, so the wait for the prefetched column at the end of that iteration covers them (and hipcc's wait-count pass, which knows
// that these loads write LDS, puts an s_waitcnt vmcnt(n) in front of the reads where it cannot see that); two buffers per wave take turns.  The buffers live in the LDS of the chain blocks' hand-over slots, which a
// workgroup of solo units does not use.
static constexpr int OWN_LDS_BYTES = 9 * 512;      // one buffer: nine populations x 512 bytes
typedef __attribute__((address_space(3))) void *lds_void_p;
template <typename T, int S, bool OVL = false>
__device__ __forceinline__ void own_prefetch(const MarchAddr<T, S> &a, int col, char *buf)
{
    static_assert(64 * S * sizeof(T) == 512, "one population of a window's column is 512 bytes");
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const unsigned soff = lat_off(a, k, col, 0) - (OVL ? 256u : 0u);      // (OVL: a.voff_dma is kept 256 bytes high, k_march3)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(a.rs, (lds_void_p)(buf + 512 * k), 4, a.voff_dma, soff, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(a.rs, (lds_void_p)(buf + 512 * k), 4, a.voff_dma, soff, 256, 0);
    }
}
template <typename T, int S>
__device__ __forceinline__ MV<T, S> own_read(const char *buf, int k, int lane)
{
    MV<T, S> o;
    const u2v x = *reinterpret_cast<const u2v *>(buf + 512 * k + 8 * lane);
    __builtin_memcpy(&o, &x, 8);
    return o;
}

// Step 1 of column x -> G (all nine directions).  `in` holds the streamed inputs of column x (modified in place).
// OWN_LDS: the column's own populations (general columns only) are in the LDS buffer `own_buf`, requested by own_prefetch — one iteration ago in the
// units' loops, just now for a unit's first columns; false (the two-step passes, march_unit at DEPTH 2, and the chain units): they are loaded here.
// `pre` (optional): the column's solid flags and bounce codes {solid4, code4}, fetched ahead by the caller (SiteBytes below)
template <bool BODY, int FD, typename T, int S, bool OWN_LDS = false>
__device__ __forceinline__ void march_step1(const MarchParams<T> &p, const MarchAddr<T, S> &a, int x, int j0, bool far_win, bool nonfast, bool allsolid,
                                            const T (&feq0)[9], MV<T, S> (&in)[9], MV<T, S> (&G)[9], const uint32_t *pre = nullptr, const char *own_buf = nullptr)
{
    MV<T, S> mac[3];
    if (BODY) {
        const Geom &g = p.g;
        const int gi = x + g.gi0;
#ifdef WT_EXP_NO_OWN       // timing experiment (WRONG results): what do the stage-1 loads of a general column's own populations cost?
        auto own = [&](int k) { return in[k]; };
#else
        auto own = [&](int k) {
            if constexpr (OWN_LDS) return own_read<T, S>(own_buf, k, a.lane);
            else return bload<T, S>(a.rs, a.voff, lat_off(a, k, x, 0));
        };
#endif
        if (__builtin_expect(gi <= 0 || gi >= g.nx_g - 1 || nonfast, 0)) {
            // rare paths (scalar branches): inlet / outlet columns, body surface, body interior
            uint32_t solid4 = 0, code4 = 0;
            if (nonfast) {
                if (pre) { solid4 = pre[0]; code4 = pre[1]; }
                else {
                    solid4 = load_site_bytes<S>(p.mask + (long)(x + 1) * g.pitch + site_row<S, (FD & MARCH_FD_OVL) != 0>(j0, g.ny));
                    code4 = load_site_bytes<S>(p.bcode + (long)x * g.pitch + site_row<S, (FD & MARCH_FD_OVL) != 0>(j0, g.ny));
                }
            }
            const bool any_solid = __ballot(solid4 != 0) != 0ULL;
            if (gi <= 0) {
#pragma unroll
                for (int k = 0; k < 9; k++) G[k] = mv_splat<T, S>(feq0[k]);
            } else if (gi >= g.nx_g - 1) {
#pragma unroll
                for (int k = 0; k < 9; k++) G[k] = bload<T, S>(a.rs, a.voff, lat_off(a, k, x - 1, 0));
            } else if (allsolid) {
#pragma unroll
                for (int k = 0; k < 9; k++) G[k] = own(opp_of(k));
                return;
            } else {
                march_bounce<T, S>(in, code4, own);
                march_collide_general<T, S, FD, false>(in, solid4, j0, g.ny, p.fdv, p.tau, p.U0, feq0, G, mac);
                return;
            }
            if (any_solid) march_solid<T, S, false>(G, mac, solid4, own);      // inlet / outlet columns with solid sites
            return;
        }
    }
    march_collide<T, S, FD, false>(in, p.fdv, p.tau, G, mac);
    if (far_win) march_far_rows<T, S, false>(j0, p.g.ny, p.U0, feq0, G, mac);
}

// ------------------------------------------------------------------------------------------------
// host side: the unit lists of one mask
// ------------------------------------------------------------------------------------------------
// Marched column range of a handle: global edges are part of the march (inlet column 0; outlet column emitted with NX-2), local slab edges are
// not (their ghost columns lose two columns of validity per two-step pass).  The range of two-step tables; march_range3 (step_march3.hpp) gives
// that of any depth.
struct MarchRange { int i_begin, i_end, outlet_after; };
static inline MarchRange march_range(const Geom &g)
{
    MarchRange r;
    r.i_begin = (g.gi0 == 0) ? 0 : 1;
    r.i_end = g.nxl - 1;
    r.outlet_after = (g.gi0 + g.nxl == g.nx_g) ? 1 : 0;
    return r;
}

struct MarchPlan {
    std::vector<MarchUnit> units;
    int nwin = 0;
    int chunk = 0;       // columns of a typical unit
};

// wcls: host copy of the window-tile classes [nwin][nxl+2].  All units of a launch run side by side in whole
// "rounds" of `slots` resident waves and take about equally long, so the launch time is rounds x unit time:
// a unit count just above a multiple of `slots` wastes most of a round (measured on 4096^2: 4096 units 126 us
// per step, 4298 units 162 us).  The marched columns of every window are therefore cut into units of equal
// COST — a FAST column costs 1, any other column 1 + alpha (its step 1 waits for nine more loads) — such that
// the total is at most `target_units` (a multiple of `slots` chosen by the caller), or, when max_cost > 0, into
// units of at most max_cost (tests, experiments).
// min_last: least number of marched columns of a window's LAST unit (a four-step pass needs 2: the unit before the outlet unit
// must end two columns short of the outlet column); max_len: most columns of a unit; parts_multiple: the units of a window come in
// whole groups of that many where the window has at least one group (step_chain.hpp: blocks of four).
static inline MarchPlan build_march_plan(const uint8_t *wcls, const Geom &g, int win, long target_units, int max_cost = 0, double alpha = 1.0,
                                         const MarchRange *range = nullptr, int min_last = 1, int max_len = MARCH_MAX_CHUNK, int parts_multiple = 1)
{
    MarchPlan pl;
    const int nwin = march_nwin(g.ny, win), ld = g.nxl + 2;
    pl.nwin = nwin;
    const MarchRange r = range ? *range : march_range(g);
    const int ncol = r.i_end - r.i_begin;
    if (ncol <= 0) return pl;
    std::vector<double> wcost((size_t)nwin, 0.0);
    double total = 0.0;
    for (int w = 0; w < nwin; w++) {
        const uint8_t *c = wcls + (size_t)w * ld + 1;
        for (int x = r.i_begin; x < r.i_end; x++) wcost[w] += (c[x] == WC_FAST) ? 1.0 : 1.0 + alpha;
        total += wcost[w];
    }
    double target;       // cost of one unit
    if (max_cost > 0) target = (double)max_cost;
    else {
        if (target_units < nwin) target_units = nwin;
        target = total / (double)target_units;
    }
    if (target > (double)max_len) target = (double)max_len;      // the kernel's unit length limit (MARCH_MAX_CHUNK / MARCH3_MAX_CHUNK)
    if (target < 1.0) target = 1.0;
    pl.chunk = (int)(target + 0.5);
    for (int w = 0; w < nwin; w++) {
        const uint8_t *c = wcls + (size_t)w * ld + 1;
        // whole parts only, never more than wcost / target of them: the total stays <= target_units
        int parts = (int)(wcost[w] / target);
        if (max_cost > 0) parts = (int)((wcost[w] + target - 1e-9) / target);
        if (parts < 1) parts = 1;
        if (max_cost <= 0 && parts_multiple > 1 && parts >= parts_multiple && (ncol + parts - 1) / parts < max_len) parts -= parts % parts_multiple;
        const double per = wcost[w] / parts;
        int ia = r.i_begin, done = 0;
        double acc = 0.0;
        for (int x = r.i_begin; x < r.i_end; x++) {
            acc += (c[x] == WC_FAST) ? 1.0 : 1.0 + alpha;
            const bool last = (x + 1 == r.i_end);
            const bool tail_short = !last && r.i_end - (x + 1) < min_last;      // a cut here would leave too short a last unit
            if (last || (!tail_short && ((done + 1 < parts && acc >= per * (done + 1) - 1e-9) || x + 1 - ia >= max_len))) {
                pl.units.push_back(MarchUnit{ia, x + 1, w, (r.outlet_after && last) ? MU_OUTLET_AFTER : 0});
                ia = x + 1;
                done++;
            }
        }
    }
    // chunk-major order: the windows of one chunk are neighbours in the list (adjacent waves read adjacent kilobytes)
    std::stable_sort(pl.units.begin(), pl.units.end(), [](const MarchUnit &x, const MarchUnit &y) { return x.ia != y.ia ? x.ia < y.ia : x.w < y.w; });
    return pl;
}

// The same cut by TIME instead of by owned columns.  All units of a launch are resident together (whole rounds), so the launch takes as
// long as its slowest unit, and a unit's time is the cost of every column it ITERATES over — its own and the `over` columns it recomputes
// for its neighbours' sake (pipeline fill and drain: 2.7 iterations of a three-step pass, 4.5 of a four-step one), which in the body zone
// are body columns too (per-unit clocks, tools/unit_clocks.py: with the cut by owned columns a two-column body unit of the bench mask took
// 1.55 x as long as a ten-column plain one and set the pace of the whole launch).  time(ia, ib) = C(ib + over / 2) - C(ia - over / 2) with
// C the running cost of the window's columns (a FAST column 1, a column of an all-solid tile 1 + alpha_solid, any other 1 + alpha, nothing beyond the tunnel's ends) and `tail` more
// for the unit that also emits the outlet column; the smallest t for which every window cut greedily into units of time <= t gives at
// most target_units in total is found by bisection.
static inline MarchPlan build_march_plan_timed(const uint8_t *wcls, const Geom &g, int win, long target_units, double alpha, const MarchRange &r, int min_last,
                                               int max_len, double over, double tail, double alpha_solid, const float *colw = nullptr)
{
    MarchPlan pl;
    const int nwin = march_nwin(g.ny, win), ld = g.nxl + 2;
    pl.nwin = nwin;
    const int ncol = r.i_end - r.i_begin;
    if (ncol <= 0) return pl;
    if (target_units < nwin) target_units = nwin;
    const int E = (int)(over / 2) + 2;                         // columns beyond the marched range that enter a unit's time
    const int n = ncol + 2 * E;
    std::vector<double> C((size_t)nwin * (n + 1), 0.0);        // C[w][k] = cost of columns i_begin - E .. i_begin - E + k - 1
    for (int w = 0; w < nwin; w++) {
        const uint8_t *c = wcls + (size_t)w * ld + 1;
        double *Cw = &C[(size_t)w * (n + 1)];
        for (int k = 0; k < n; k++) {
            const int x = r.i_begin - E + k, gi = x + g.gi0;
            double cost = 0.0;
            if (gi >= 0 && gi < g.nx_g) cost = (x >= -1 && x <= g.nxl && c[x] != WC_FAST) ? 1.0 + (c[x] == WC_SOLID ? alpha_solid : alpha) : 1.0;
            if (colw && x >= -1 && x <= g.nxl) cost *= colw[(size_t)w * ld + x + 1];      // measured correction (tune_fuse_plan)
            Cw[k + 1] = Cw[k] + cost;
        }
    }
    auto Cf = [&](const double *Cw, double x) {                // running cost up to (fractional) column x
        double k = x - (r.i_begin - E);
        if (k < 0) k = 0;
        if (k > n) k = n;
        const int k0 = (int)k;
        return k0 >= n ? Cw[n] : Cw[k0] + (k - k0) * (Cw[k0 + 1] - Cw[k0]);
    };
    auto unit_time = [&](const double *Cw, int ia, int ib) {
        return Cf(Cw, ib + over / 2) - Cf(Cw, ia - over / 2) + ((r.outlet_after && ib == r.i_end) ? tail : 0.0);
    };
    // cut one window for a time limit t; returns the number of units (and the cuts when `out` is given)
    auto cut = [&](int w, double t, std::vector<MarchUnit> *out) {
        const double *Cw = &C[(size_t)w * (n + 1)];
        int ia = r.i_begin, count = 0;
        while (ia < r.i_end) {
            int ib = ia + 1;
            const int cap = std::min(r.i_end, ia + max_len);
            while (ib < cap && unit_time(Cw, ia, ib + 1) <= t) ib++;
            if (r.i_end - ib > 0 && r.i_end - ib < min_last) {     // too short a last unit: take it in, or leave it min_last columns
                if (r.i_end - min_last <= ia || (r.i_end - ia <= max_len + min_last - 1 && unit_time(Cw, ia, r.i_end) <= t)) ib = r.i_end;
                else ib = r.i_end - min_last;
            }
            if (out) out->push_back(MarchUnit{ia, ib, w, (r.outlet_after && ib == r.i_end) ? MU_OUTLET_AFTER : 0});
            ia = ib;
            count++;
        }
        return count;
    };
    auto total = [&](double t) { long s = 0; for (int w = 0; w < nwin; w++) s += cut(w, t, nullptr); return s; };
    double lo = 0.0, hi = (double)max_len * (1.0 + alpha) + over * (1.0 + alpha) + tail + 1.0;
    if (total(hi) > target_units) lo = hi;                     // the length cap forces more units than asked for: longest units
    else {
        for (int it = 0; it < 24; it++) {       // (t to 6e-8 of its range: unit counts change at discrete t)
            const double mid = 0.5 * (lo + hi);
            if (total(mid) <= target_units) hi = mid; else lo = mid;
        }
    }
    const double t = hi;
    pl.chunk = 0;
    for (int w = 0; w < nwin; w++) cut(w, t, &pl.units);
    long cols = 0;
    for (const MarchUnit &u : pl.units) cols += u.ib - u.ia;
    pl.chunk = pl.units.empty() ? 0 : (int)((double)cols / (double)pl.units.size() + 0.5);
    // chunk-major order: the windows of one chunk are neighbours in the list (adjacent waves read adjacent kilobytes)
    std::stable_sort(pl.units.begin(), pl.units.end(), [](const MarchUnit &x, const MarchUnit &y) { return x.ia != y.ia ? x.ia < y.ia : x.w < y.w; });
    return pl;
}

}  // namespace wt
