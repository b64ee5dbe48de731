// polar.hip — C-ABI implementation of libwtpolar.so (see include/wt_polar.h): B independent tunnels of one size
// ("members") advanced by one launch per step, with the force reduction of every member on the device.
//
// Bit identity with a libwindtunnel handle holds by construction: each member keeps wt_create's layout (pitch, pad
// columns, plane stride), its tiles are classified by the same k_classify, a batched step runs the same step_tile
// (step_fast.hpp) with tau and U0 rounded to the storage type on the host as wt_step rounds them, and a force sample
// runs k_forces' block body (forces_block, kernels.hpp) over wt_forces' block count, summed over the blocks in the
// same order in double.
//
// Surface loads (wtp_enable_loads) are a reduction of their own, k_loads_batch, launched behind k_forces_batch: the pitching
// moment of the force model's faces about a per-member point and the running sums of rho above and below the body, one
// wave per (member, column).  It shares nothing with the force reduction, whose values it leaves as they are.
//
// Momentum exchange (wtp_enable_mex) is a third reduction, k_mex_batch, launched behind the other two: the force and the moment
// that the half-way bounce-back links hand to the body, summed from the populations of the lattice the step wrote.  It reads
// the lattice and the mask and writes buffers of its own.
//
// All three end the same way: the last block of a member to finish (member_done) adds the member's partials in index order, so
// that a sample does not depend on the order in which the blocks ran, and writes one row of a SampleTable.
//
// Mean fields (wtp_enable_mean) are no reduction: k_mean_batch, launched behind the three, streams every member's emitted rho,
// ux, uy once and adds them and their products to seven planes of running sums, one owner thread per entry.
//
// Probe points (wtp_enable_probes) are no reduction either: k_probe_batch, launched behind the four, samples every member's emitted rho,
// ux, uy at the member's own points, bilinearly between cell centres, and adds the three values of each point to its running sums, one
// owner lane per point.  A batch that never enables them launches the kernels it always launched.
//
// The step has one tiled kernel, k_step_batch<T, EMIT, LOADMODE, COLL, WALL, FAR>: step_tile (step_fast.hpp) of the wave's tile with
// the collision, the wall rule and the far field as template arguments, and the values each of them reads per member in one argument
// whose members exist only in the variants that read them (StepModel).  The models below select among its instantiations.
//
// The Smagorinsky subgrid viscosity (wtp_enable_les) is no read-out but another collision: while it is on, wtp_step launches
// k_step_batch with COLLIDE_LES, the same step_tile with collide_les in its interior cells and one more value per member.  A batch
// that has it off launches the plain instantiation with the arguments it always had.
//
// Interpolated bounce-back (wtp_enable_ibb) is another wall rule: while it is on, wtp_step launches k_step_batch with WALL_INTERP, the same
// step_tile with wall_incoming at the links of its general tiles and eight planes of wall distances per member, with either
// collision, and a sample's momentum exchange comes from k_mex_batch with LinkInterp, the same reduction with the interpolated link
// rule.  A batch that has it off launches the kernels it always launched, with the arguments they always had.
//
// Wall velocity (wtp_enable_wall_velocity) is a third wall rule on top of the second: while it is on, wtp_step launches k_step_batch with
// WALL_MOVING: the same step_tile with the moving-wall overload of wall_incoming at the links of its general tiles and eight more planes per
// member, the wall-normal velocities, read on the lanes that read a wall distance, with every collision and every far field, and a sample's
// momentum exchange comes from k_mex_batch with LinkMoving.  Native storage only.  A batch that has it off launches the
// kernels it always launched, with the arguments they always had.
//
// The inclined free stream (wtp_enable_wind) is another far field: while it is on, wtp_step launches k_step_batch with FAR_INCLINED, the same
// step_tile with feq(1, U0, V0) in its far-field cells and one more value per member, with either collision and either wall rule,
// and wtp_init_equilibrium fills the members by k_fill_wind.  A batch that has it off launches the kernels it always launched, with
// the arguments they always had.
//
// Half-precision population storage (wtp_create_stored with WTP_STORE_HALF) is another storage of an fp32 batch: its lattices hold
// each population as the binary16 deviation from its lattice weight, in wt_create's layout with 2-byte elements.  wtp_step launches
// k_step_half_batch<EMIT, COLL, FAR>, site_general with half_t as its stored element: a Load in front of its branches and a Store behind,
// fp32 between, with every collision and either far field, and k_step_batch's model argument; wtp_init_equilibrium fills by k_fill_half and a sample's momentum exchange comes from k_mex_batch with half_t elements.  The other
// read-outs read the fp32 macroscopic planes and run unchanged.  A native batch launches the kernels it always launched, with the
// arguments they always had.
//
// State upload (wtp_write_f, wtp_write_stored) is the inverse of the read-backs: a member's [9][NY][NX] host planes go through the stage
// into its current lattice by k_rows_to_cols, or by k_half_rows_to_cols with a Store on the way.  A write marks the macroscopic planes
// stale until a step has emitted and zeroes the member's running sums; with wtp_set_step_count a sweep continues where another stopped.
// A batch that never writes launches the kernels it always launched.
//
// The two-relaxation-time collision (wtp_enable_trt) is a third collision: while it is on, wtp_step launches k_step_batch (in a half
// batch k_step_half_batch) with COLLIDE_TRT or COLLIDE_TRT_LES, the same step_tile (site_general) with collide_trt in its interior cells and one more value per member,
// the magic number, without or with the Smagorinsky eddy viscosity, with either wall rule and either storage.  Its instantiations always take
// the inclined far field, with an array of zeros as the cross-flow while wtp_enable_wind is off.  While it is on, wtp_step refuses a
// tau that is not above 0.5 in the batch's dtype.  A batch that has it off launches the kernels it always launched, with the arguments
// they always had.
//
// The prescribed far-field profile (wtp_enable_far_profile) is a third far field: while it is on, wtp_step launches
// k_step_batch with FAR_PROFILE, the same step_tile with feq(rho, ux, uy) of the cell's entry in the member's tables in its far-field cells, with
// every collision and either wall rule.  wtp_set_far_profile checks the tables on the host and uploads them; wtp_step refuses to run
// while a member has none.  Native storage only.  A batch that has it off launches the kernels it always launched, with the arguments
// they always had.
//
// The device-side far-field vortex (wtp_enable_far_vortex) is an owner of those tables: while it is on, the stepping loop follows every
// `every`-th step by k_forces_batch into a scratch row and one launch of k_far_vortex, which moves every member's vortex and source
// strength by the force, clips them and rebuilds the member's three tables, all in stream order, and logs the update.  The step kernels
// do not know who wrote the tables.  A batch that has it off launches the kernels it always launched.
//
// Every variant above is an instantiation of its own, so a batch runs the code object its switches select and no other.  What the
// variants share is source text: one site (site_general, kernels.hpp, for every storage), one tiled step kernel and one half step kernel
// with one selection and one launch on the host (with_step_variant, step_model), one momentum-exchange kernel (k_mex_batch, with a link
// rule per wall rule), one stepping loop on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/wt_polar.h"
#include "errors.hpp"       // g_err, fail, HIP_TRY, WT_TRY
#include "kernels.hpp"
#include "step_fast.hpp"

using namespace wt;

static const int kLoadsWaves = 16;         // waves (columns) of one k_loads_batch block
static const int kTicketStride = 32;       // unsigned ints between the members' k_loads_batch / k_mex_batch tickets: one 128-byte line each
#ifndef WTP_MEX_WINDOW
#define WTP_MEX_WINDOW 1                   // 1: k_mex_batch visits a member's body columns only; 0: every interior column (measurements)
#endif

#ifndef WTP_MEAN_ROWS
#define WTP_MEAN_ROWS 2                    // rows of a column that one lane of k_mean_batch owns: 2 = 16-byte accesses to the sums; 1 = 8-byte ones (measurements)
#endif
static const int kMeanPlanes = 7;          // sums of rho, ux, uy, rho rho, ux ux, uy uy, ux uy, in wtp_mean_sums' order

struct MexPartial { double fx, fy, mz; long long links; };     // one column's sums of k_mex_batch
template <typename V, int R> using RowRun = V __attribute__((ext_vector_type(R)));     // R consecutive rows of one column: one load or store

// Element strides between consecutive members of each array.  Every stride is rounded to 4 KiB and grown by 17 KiB, as
// wt_create's plane stride is, so that the members' lattices do not all start on the same HBM channels.
struct MemberStrides { long lat, macro, mask, tiles; };

static long member_stride(size_t bytes, size_t esz) { return (long)(((bytes + 4095) / 4096 * 4096 + 17408) / esz); }

// A feature's optional device buffers, all or none: every *p of `want` that is still null is allocated with its bytes (one that is held,
// from an earlier call, is kept), and only when all of them succeeded are they assigned.  On a failure what was got is freed, nothing is
// assigned and HIP's last error is cleared, so that the batch goes on as it was and later launches do not see the error.
struct DevBuf { void **p; size_t bytes; };

static int alloc_all(const std::vector<DevBuf> &want, const char *what)
{
    std::vector<void *> got;
    size_t total = 0;
    hipError_t e = hipSuccess;
    for (const DevBuf &w : want) if (!*w.p) total += w.bytes;
    for (const DevBuf &w : want) {
        void *p = nullptr;
        if (*w.p) continue;
        if ((e = hipMalloc(&p, w.bytes)) != hipSuccess) break;
        got.push_back(p);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void *p : got) (void)hipFree(p);
        return fail(e == hipErrorOutOfMemory ? WT_ERR_OOM : WT_ERR_HIP, "the %s (%zu bytes) could not be allocated: %s", what, total, hipGetErrorString(e));
    }
    size_t k = 0;
    for (const DevBuf &w : want) if (!*w.p) *w.p = got[k++];
    return WT_OK;
}

// The samples of one read-out: up to four columns of 8-byte values (double or long long), [cap + 1][B] each, one value per
// member and row.  Rows [0, cap) are the history, in step order; row cap is the scratch row of the on-demand call.
struct SampleTable {
    void *col[4] = {nullptr, nullptr, nullptr, nullptr};
    int ncols = 0;
    size_t rows = 0, members = 0;

    size_t bytes() const { return rows * members * 8; }
    bool allocated() const { return ncols > 0 && col[ncols - 1]; }
    int alloc(int n, size_t cap, size_t B, const char *what)      // (columns already held are kept)
    {
        ncols = n; rows = cap + 1; members = B;
        std::vector<DevBuf> want;
        for (int c = 0; c < n; c++) want.push_back({&col[c], bytes()});
        return alloc_all(want, what);
    }
    // "Never sampled" in every row of the columns of `mask` (bit c: column c): bytes 0xFF, a NaN as a double, -1 as a long long.
    int fill(unsigned mask, hipStream_t st)
    {
        for (int c = 0; c < ncols; c++) if (mask >> c & 1u) HIP_TRY(hipMemsetAsync(col[c], 0xFF, bytes(), st));
        return WT_OK;
    }
    // Column c of row `row` on the device: what a launch writes.
    template <typename V> V *at(int c, int row) const
    {
        static_assert(sizeof(V) == 8, "a sample is 8 bytes");
        return reinterpret_cast<V *>(col[c]) + (size_t)row * members;
    }
    // Rows [first, first + count) of every column whose destination is not null, to the host.
    int read(int first, int count, void *const *dst) const
    {
        const size_t n = (size_t)count * members * 8;
        for (int c = 0; c < ncols && n; c++) if (dst[c]) HIP_TRY(hipMemcpy(dst[c], at<double>(c, first), n, hipMemcpyDeviceToHost));
        return WT_OK;
    }
    void release() { for (void *&p : col) { if (p) (void)hipFree(p); p = nullptr; } }
};

// The per-batch settings of the device-side far-field vortex (include/wt_polar.h "Device-side far-field vortex"), by value to its kernel:
// den = (2 pi) u_ref and bound = min(xc - 0.5, yc - 0.5, NY - 0.5 - yc), both formed on the host.
struct VortexSet { double relax, den, bound, xc, yc; int with_source; };
static const int kVortexBlock = 256;       // table entries (lanes) of one k_far_vortex block

struct wtp_batch {
    int nx = 0, ny = 0, dtype = WT_F32, device = 0, members = 0, cap = 0;
    size_t esz = 4;
    int storage = WTP_STORE_NATIVE;      // WTP_STORE_HALF: the lattices hold binary16 deviations from the weights (fp32 batches only)
    size_t lat_esz = 4;                  // bytes of one stored population: esz, or 2 in a half batch
    Geom g{};
    int tiles_per_col = 0;
    MemberStrides ms{};
    void *f[2] = {nullptr, nullptr};     // members' lattices, each laid out as wt_create's
    int cur = 0;
    void *macro = nullptr;
    uint8_t *mask = nullptr;
    uint8_t *tiles = nullptr;
    void *params = nullptr;              // [B][2] of T: tau, U0 of the last stepping call
    std::vector<double> params_host;     // ... as the caller gave them (doubles), to skip unchanged uploads
    // Smagorinsky subgrid viscosity (wtp_enable_les); the pointer is null until then
    bool les = false;
    void *les_c = nullptr;               // [B] of T: c = 18 sqrt(2) Cs^2 of every member
    // interpolated bounce-back (wtp_enable_ibb); the pointer is null until then
    bool ibb = false;
    void *wq = nullptr;                  // [B][8] planes of T laid out like population planes 1..8, members q_stride elements apart
    long q_stride = 0;
    // wall velocity (wtp_enable_wall_velocity), on top of interpolated bounce-back; the pointer is null until then
    bool wallvel = false;
    void *wu = nullptr;                  // [B][8] planes of T laid out like wq, members q_stride elements apart
    // inclined free stream (wtp_enable_wind); the pointer is null until then
    bool wind = false;
    void *wind_v = nullptr;              // [B] of T: the cross-flow V0 of every member
    std::vector<double> wind_host;       // ... as the caller gave them (doubles), for wtp_init_equilibrium
    // two-relaxation-time collision (wtp_enable_trt); the pointers are null until then
    bool trt = false;
    void *trt_lam = nullptr;             // [B] of T: the magic number of every member
    void *zero_v = nullptr;              // [B] of T, all zero: the cross-flow its kernels read while the free stream is axial
    // prescribed far-field profile (wtp_enable_far_profile); the pointer is null until then
    bool profile = false;
    void *prof = nullptr;                // [B] tables of T (FarProfile, d2q9.hpp), members p_stride elements apart
    long p_stride = 0;
    int p_nxp = 0;                       // elements per plane of `bottom` and `top`: NX rounded up to 64
    std::vector<uint8_t> prof_set;       // [B]: the member has been given a profile (wtp_set_far_profile)
    // device-side far-field vortex (wtp_enable_far_vortex); every pointer is null until then
    bool vortex = false;
    VortexSet v_set{};                   // the per-batch settings the update kernel reads
    int v_every = 0;
    long long v_after = 0, v_since = 0;  // the first absolute step count that may update; steps enqueued while the model is on since it was enabled
    double *v_member = nullptr;          // [4][B]: u_far, v_far, cos_a, sin_a
    double *v_str = nullptr;             // [2][2][B]: the strengths and the sources, double-buffered; v_str[v_par] holds the current ones
    int v_par = 0;
    void *v_forces = nullptr;            // [4][B] of 8 bytes: the scratch row of the update's force read-out (fx, fy, surf, rev)
    double *v_log = nullptr;             // [4][v_cap][B]: fx, fy, strength, source of every update
    int32_t *v_clip = nullptr;           // [v_cap][B]: the update clipped
    int v_cap = 0;
    std::vector<int64_t> v_step;         // step count of each log row held
    ForcePartial *partials = nullptr;    // [B][nb]
    unsigned int *tickets = nullptr;     // [B]: blocks of a member's reduction done (reset by its last block)
    SampleTable forces;                  // fx, fy (double), surf, rev (long long)
    std::vector<int64_t> h_step;         // step count of each history row held, in every table
    void *stage = nullptr;               // layout conversion (one member's plane, or one mask)
    size_t stage_bytes = 0;
    int nb = 0;                          // blocks of one member's force reduction
    hipStream_t st = nullptr;
    std::vector<uint8_t> mask_set;
    std::vector<int32_t> surf_rows;      // [B][2][NX]: rows of the fluid cells above / below each column's body (-1: none), from the masks
    // surface loads (wtp_enable_loads); every pointer is null until then
    bool loads = false;
    double *l_ref = nullptr;             // [B][2]: xref, yref
    double *l_col = nullptr;             // [B][NX]: the columns' moment partials of the running reduction
    unsigned int *l_tickets = nullptr;   // [B] tickets, kTicketStride apart
    SampleTable moment;                  // mz (double)
    double *s_rho = nullptr;             // [B][2][NX]: sums of rho over the samples, upper then lower
    long long *s_cnt = nullptr;          // [B][2][NX]: samples added
    // momentum exchange (wtp_enable_mex); every pointer is null until then
    bool mex = false;
    std::vector<int32_t> mex_win;        // [B][2]: first column that can own a link and the number of such columns, from the masks
    int32_t *x_win = nullptr;            // ... on the device
    double *x_ref = nullptr;             // [B][2]: xref, yref
    MexPartial *x_col = nullptr;         // [B][NX]: the columns' partials of the running reduction
    unsigned int *x_tickets = nullptr;   // [B] tickets, kTicketStride apart
    SampleTable xforces;                 // fx, fy, mz (double), links (long long)
    // mean fields (wtp_enable_mean); every pointer is null until then
    bool mean = false;
    double *m_sums = nullptr;            // [B][7][NX][m_pitch], y fastest, members m_stride apart
    long long *m_cnt = nullptr;          // [B]: samples added
    long m_stride = 0;
    int m_pitch = 0;                     // NY rounded up to WTP_MEAN_ROWS
    // probe points (wtp_enable_probes); every pointer is null until then
    bool probes = false;
    int pb_n = 0;                        // P, the points of every member
    long long *pb_off = nullptr;         // [B][P]: the offset of cell (i0, j0) in a macroscopic plane, i0 * pitch + j0; -1: the point is inactive
    double *pb_w = nullptr;              // [B][4][P]: w00, w10, w01, w11
    double *pb_sums = nullptr;           // [B][3][P]: sums of rho, ux, uy over the samples
    long long *pb_cnt = nullptr;         // [B]: samples added
    double *pb_row = nullptr;            // [3][P]: the scratch row of wtp_probe_sample
    bool inited = false;
    bool macro_stale = false;            // a member's populations were written (wtp_write_f / wtp_write_stored) and no step has emitted since
    long long steps_done = 0;
};

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// A wave's place in a tiled step launch, the prologue of k_step_batch: blockIdx.y is the member, blockIdx.x * 4 + wave
// the tile inside it (k_step's grid).  rev walks members and tiles backwards on every other step, as k_step walks its tiles.  A wave
// past the last tile is not live and returns.
struct MemberTile {
    long ntiles, t;
    int rev;
    __device__ __forceinline__ MemberTile(const Geom &g, int tiles_per_col, int rev_)
        : ntiles((long)g.nxl * tiles_per_col), t((long)blockIdx.x * 4 + (threadIdx.x >> 6)), rev(rev_) {}
    __device__ __forceinline__ bool live() const { return t < ntiles; }
    __device__ __forceinline__ long member() const { return rev ? (long)gridDim.y - 1 - blockIdx.y : (long)blockIdx.y; }
    __device__ __forceinline__ long tile() const { return rev ? ntiles - 1 - t : t; }
};

// The model arguments of a step kernel, by value behind the arguments every variant takes: each piece exists only in the variants
// that read it, so that a variant's kernel arguments are the ones it uses and no other.  (One unused pointer argument costs the
// fp32 kernels about 30 VGPRs and two waves; see step_waves.)  In argument order:
//   cles     [B]: c = (T)(18 sqrt(2) Cs^2) of every member                                        the Smagorinsky collisions
//   wq       the members' wall distances, eight planes each, qstride elements apart               WALL_INTERP, WALL_MOVING
//   wu       the members' wall-normal velocities, eight planes each, ustride elements apart       WALL_MOVING
//   vwind    [B]: the cross-flow V0 of every member                                               FAR_INCLINED
//   lam      [B]: the magic number of every member                                                the two-relaxation-time collisions
//   prof     the members' tables (FarProfile, d2q9.hpp), pstride elements apart, nxp elements per plane of `bottom` and `top`   FAR_PROFILE
//   rev      walk members and tiles backwards (MemberTile)                                        every variant
template <typename T, bool ON> struct ArgLes { const T *__restrict__ cles; };
template <typename T, bool ON> struct ArgWallQ { const T *__restrict__ wq; long qstride; };
template <typename T, bool ON> struct ArgWallU { const T *__restrict__ wu; long ustride; };
template <typename T, bool ON> struct ArgWind { const T *__restrict__ vwind; };
template <typename T, bool ON> struct ArgTrt { const T *__restrict__ lam; };
template <typename T, bool ON> struct ArgProfile { const T *__restrict__ prof; long pstride; int nxp; };
template <typename T> struct ArgLes<T, false> {};
template <typename T> struct ArgWallQ<T, false> {};
template <typename T> struct ArgWallU<T, false> {};
template <typename T> struct ArgWind<T, false> {};
template <typename T> struct ArgTrt<T, false> {};
template <typename T> struct ArgProfile<T, false> {};
template <typename T, int COLL, int WALL, int FAR>
struct StepModel : ArgLes<T, coll_has_les(COLL)>, ArgWallQ<T, wall_has_links(WALL)>, ArgWallU<T, WALL == WALL_MOVING>, ArgWind<T, FAR == FAR_INCLINED>,
                   ArgTrt<T, coll_is_trt(COLL)>, ArgProfile<T, FAR == FAR_PROFILE> {
    int rev;
};

// Waves per SIMD that a tiled step kernel asks for (0: nothing asked, the kernels with the axial far field), from the compiler's resource
// report (profiles/polar_trt_isa.txt, profiles/polar_profile_isa.txt).  Left to itself the compiler gives every
// kernel with more arguments than the axial ones 109 to 124 VGPRs in fp32 (4 waves), whatever the far field, the collision or the wall
// rule is; an unused pointer argument added to the plain kernel does the same.
//  * inclined, single relaxation time: asked for the axial kernels' occupancy (6 waves; 5 emitting or with the Smagorinsky model; 4 in
//    fp64) it allocates 79 to 95 VGPRs, theirs within 2, without scratch, interpolated walls included.
//  * two relaxation times: the emitting and the Smagorinsky kernels allocate 84 to 92 VGPRs in fp32 (5 waves) and 108 to 122 in fp64
//    (4 waves) without scratch, but the plain non-emitting fp32 kernels, asked for 6 waves, get 80 VGPRs and 12 to 16 bytes of scratch
//    per lane: the split keeps n[k], the half-sums and the half-differences alive together.  So every fp32 kernel asks for 5.
//  * profile: every kernel asks for what its inclined twin asks for and allocates 79 to 94 VGPRs in fp32 and 93 to 111 in fp64 without
//    scratch (the entry of a FAST tile's far row is loaded behind the collision, so it adds no live register to it).  One exception: the
//    plain non-emitting fp32 kernel with interpolated walls, asked for its twin's 6 waves, got 79 VGPRs and 12 bytes of scratch per lane
//    where the twin has none, so it asks for 5.
//  * moving walls: every kernel asks for what its interpolating twin asks for and allocates 79 to 95 VGPRs in fp32 and 83 to 119 in fp64
//    without scratch (profiles/polar_wallvel_isa.txt): the velocity is loaded on a link's lanes, behind the ballot, and dies in
//    wall_incoming.  The same exception holds: asked for 6 waves, the plain non-emitting fp32 profile kernel got 79 VGPRs and 12 bytes of
//    scratch per lane, so it asks for 5 like its twin.
template <typename T, bool EMIT, int COLL, int WALL, int FAR>
constexpr int step_waves()
{
    if (FAR == FAR_AXIAL) return 0;
    if (sizeof(T) == 8) return 4;
    if (EMIT || COLL != COLLIDE_BGK) return 5;
    return FAR == FAR_PROFILE && wall_has_links(WALL) ? 5 : 6;
}

// One step of every member: step_tile (step_fast.hpp) of the wave's tile (MemberTile) with the member's tau and U0, on the member's
// lattices, planes, mask and tile classes.  COLL, WALL and FAR are step_tile's: the collision of the interior fluid cells, the wall rule
// and the far field; `a` holds what they read per member (StepModel).  A member with cles = 0, with wall distances that are all 0.5, with
// V0 = 0 or with a profile that holds (1, U0, V0) in every entry computes the bits of the variant without that model.
// The far fields (include/wt_polar.h "Inclined free stream", "Prescribed far-field profile"): in the step, a far-field cell is one that
// is not solid, not in the outlet column, and lies in column 0, row 0 or row NY-1.  With FAR_INCLINED such a cell writes
// feq_k(1, U0, V0) and stores (1, U0, V0), feq being feq_all, V0 = vwind[m]; with FAR_PROFILE it writes feq_k(rho, ux, uy) of its entry
// in the member's tables and stores (rho, ux, uy), and U0 is not read by such a cell.  The branch order (solid, then outlet, then far
// field, then interior) does not change, and nothing else in the step changes.
// The two-relaxation-time collisions are not built with FAR_AXIAL: a batch without wtp_enable_wind hands them an array of zeros as
// vwind, and V0 = 0 gives the axial far field's bits because ex*U0 + ey*0 and U0*U0 + 0*0 are exact, so that the collision costs
// eight instantiations per dtype and not sixteen.
template <typename T, bool EMIT, int LOADMODE, int COLL, int WALL, int FAR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(step_waves<T, EMIT, COLL, WALL, FAR>())))
void k_step_batch(const T *__restrict__ fs, T *__restrict__ fd, T *__restrict__ macro, const uint8_t *__restrict__ mask,
                  const uint8_t *__restrict__ tiles, int tiles_per_col, Geom g, MemberStrides ms, const T *__restrict__ params,
                  StepModel<T, COLL, WALL, FAR> a)
{
    const int lane = threadIdx.x & 63;
    const MemberTile w(g, tiles_per_col, a.rev);
    if (!w.live()) return;
    const long m = w.member();
    const T tau = params[2 * m], U0 = params[2 * m + 1];
    T c = T(0.0), V0 = T(0.0), magic = T(0.0);
    const T *q = nullptr, *u = nullptr;
    FarProfile<T> fp;
    if constexpr (coll_has_les(COLL)) c = a.cles[m];
    if constexpr (wall_has_links(WALL)) q = a.wq + m * a.qstride;
    if constexpr (WALL == WALL_MOVING) u = a.wu + m * a.ustride;
    if constexpr (FAR == FAR_INCLINED) V0 = a.vwind[m];
    if constexpr (coll_is_trt(COLL)) magic = a.lam[m];
    if constexpr (FAR == FAR_PROFILE) { fp.tab = a.prof + m * a.pstride; fp.pitch = g.pitch; fp.nxp = a.nxp; }
    step_tile<T, EMIT, LOADMODE, false, COLL, WALL, FAR>(fs + m * ms.lat, fd + m * ms.lat, macro + m * ms.macro, mask + m * ms.mask,
                                                         tiles + m * ms.tiles, tiles_per_col, g, 0, tau, U0, w.tile(), lane, 0, 0, 0,
                                                         c, q, V0, magic, fp, u);
}

// The start state of a member with an inclined free stream: k_fill_equilibrium's walk and stores (both lattices, pad columns included), with
// the nine values of wind_init and (1, u0, v0) in the macroscopic planes.
template <typename T>
__global__ void k_fill_wind(T *__restrict__ f0, T *__restrict__ f1, T *__restrict__ macro, Geom g, Init9<T> iv, T v0)
{
    const long n = g.plane;
    const long mp = (long)g.nxl * g.pitch;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 9; k++) { f0[k * n + t] = iv.v[k]; f1[k * n + t] = iv.v[k]; }
        if (t < mp) { macro[t] = T(1.0); macro[mp + t] = iv.u0; macro[2 * mp + t] = v0; }
    }
}

// ------------------------------------------------------------------------------------------
// half-precision population storage (wtp_create_stored with WTP_STORE_HALF; include/wt_polar.h "Half-precision population storage")
// ------------------------------------------------------------------------------------------
// Definition:
//   Weights.  w_k are the fp32 weights as feq_all forms them: 4.0f/9.0f for k = 0, 1.0f/9.0f for k = 1..4, 1.0f/36.0f for
//   k = 5..8, each one fp32 division.
//   Store.  h = RN16(f - w_k): one fp32 subtraction, then one conversion to IEEE binary16, round-to-nearest-even.  Subnormal
//   halves are kept; nothing is flushed and nothing is scaled.
//   Load.  f = (float)h + w_k: an exact conversion and one fp32 addition.
//   Step.  Every population a step reads goes through Load and every population it writes goes through Store, in every branch:
//   solid (the swap), outlet (the copy), far field (the equilibrium), interior.  Everything between is the fp32 step, operation
//   for operation: gather, half-way bounce-back, moments, the net, the collision.  The macroscopic planes stay fp32 and hold what
//   the fp32 arithmetic produced.
//   Start.  wtp_init_equilibrium stores Store(v_k) of the fp32 start values it forms without the mode, including the
//   inclined-stream start; the macroscopic planes are unchanged.
// half_t, half_w, Load and Store (half_load, half_store; lat_load, lat_store with half_t elements) are d2q9.hpp's: the step, the fill,
// the transposes and the momentum exchange below all take them from there.

// Blocks of one member's k_step_half_batch grid.
static unsigned half_step_blocks(const Geom &g)
{
    const long nruns = (long)g.nxl * (g.pitch / 256);
    return (unsigned)((nruns + 3) / 4);
}

// One step of every member of a half batch: one site per lane and load, so that a wave loads 64 consecutive halves of a plane (128
// bytes) at a time.  Grid (ceil(NX * pitch / 256 / 4), B): blockIdx.y is the member, blockIdx.x * 4 + wave a run of 256 rows of one
// column, whose four chunks of 64 rows the wave walks one after the other, as k_step_batch walks a ragged tile; rev walks members and
// runs backwards on every other step, as k_step_batch walks its tiles.  There are no tile classes: every site takes site_general
// (kernels.hpp) with half_t as its stored element, which puts Load in front of its four branches and Store behind them.
// Two rows per lane with packed halves (dword loads of two rows, packed conversion, a clean pair's two sites collided in one lane,
// every other pair through the general site) was built, computed the same bits and measured slower in every walk tried, 26.9 us at best
// against 21.7 at 320x160 with 32 members (profiles/polar_half_cost.txt), and is not kept.
// COLL is the collision of the interior branch and FAR the far field, FAR_AXIAL or FAR_INCLINED, as in k_step_batch, with the same
// arguments per variant (StepModel, with float values); the two-relaxation-time collisions come with FAR_INCLINED only, as there.  fp32
// arithmetic only.  ms.lat counts halves, ms.macro floats.
template <bool EMIT, int COLL, int FAR>
__global__ __launch_bounds__(256) void k_step_half_batch(const half_t *__restrict__ fs, half_t *__restrict__ fd, float *__restrict__ macro,
                                                         const uint8_t *__restrict__ mask, Geom g, MemberStrides ms,
                                                         const float *__restrict__ params, StepModel<float, COLL, WALL_HALFWAY, FAR> a)
{
    static_assert(FAR != FAR_PROFILE && (!coll_is_trt(COLL) || FAR == FAR_INCLINED), "no profile; two relaxation times with FAR_INCLINED only");
    const int rev = a.rev;
    const int runs = (int)(g.pitch / 256);                          // runs of 256 rows in a column
    const long nruns = (long)g.nxl * runs;
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nruns) return;
    const long t = rev ? nruns - 1 - q : q;
    const int i = (int)(t / runs), j0 = (int)(t % runs) * 256;
    const long mb = rev ? (long)gridDim.y - 1 - blockIdx.y : (long)blockIdx.y;
    const float tau = params[2 * mb], U0 = params[2 * mb + 1];
    float c_les = 0.0f, V0 = 0.0f, magic = 0.0f;
    if constexpr (coll_has_les(COLL)) c_les = a.cles[mb];
    if constexpr (FAR == FAR_INCLINED) V0 = a.vwind[mb];
    if constexpr (coll_is_trt(COLL)) magic = a.lam[mb];
    const half_t *s = fs + mb * ms.lat + g.pitch;
    half_t *d = fd + mb * ms.lat + g.pitch;
    const uint8_t *m = mask + mb * ms.mask + g.pitch;
    float *mm = macro + mb * ms.macro;
    const int lane = threadIdx.x & 63;
#pragma unroll 1
    for (int v = 0; v < 4; v++) {
        const int j = j0 + v * 64 + lane;
        if (j < g.ny) site_general<float, COLL, WALL_HALFWAY, FAR>(s, d, mm, m, g, i, j, tau, U0, EMIT, c_les, nullptr, V0, magic);
    }
}

// The start state of a member of a half batch: k_fill_equilibrium's (k_fill_wind's) walk and stores, both lattices, pad columns
// included, with Store(v_k) of the nine fp32 start values and (1, u0, v0) in the macroscopic planes.
__global__ void k_fill_half(half_t *__restrict__ f0, half_t *__restrict__ f1, float *__restrict__ macro, Geom g, Init9<float> iv, float v0)
{
    const long n = g.plane;
    const long mp = (long)g.nxl * g.pitch;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 9; k++) { const half_t h = lat_store<half_t>(iv.v[k], k); f0[k * n + t] = h; f1[k * n + t] = h; }
        if (t < mp) { macro[t] = 1.0f; macro[mp + t] = iv.u0; macro[2 * mp + t] = v0; }
    }
}

// k_cols_to_rows for population plane k of a half batch: Load on the way, dst[j*W + x] = (float)src[(i0+x)*pitch + j] + w.
__global__ void k_half_cols_to_rows(const half_t *__restrict__ src, float *__restrict__ dst, int i0, int W, int ny, long pitch, float w)
{
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;   // bx: j block, by: x block
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int x = by + r, j = bx + threadIdx.x;
        if (x < W && j < ny) tile[r][threadIdx.x] = half_load(src[(long)(i0 + x) * pitch + j], w);
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int j = bx + r, x = by + threadIdx.x;
        if (x < W && j < ny) dst[(long)j * W + x] = tile[threadIdx.x][r];
    }
}

// k_rows_to_cols for population plane k of a half batch: Store on the way, dst[(i0+x)*pitch + j] = RN16(src[j*ld + x] - w).  The inverse
// walk of k_half_cols_to_rows: a 32 x 32 tile through LDS, so that the reads of the rows and the writes of the columns are both coalesced.
__global__ void k_half_rows_to_cols(const float *__restrict__ src, half_t *__restrict__ dst, int i0, int W, int ny, long pitch, long ld, float w)
{
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;   // bx: x block, by: j block
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int j = by + r, x = bx + threadIdx.x;
        if (x < W && j < ny) tile[r][threadIdx.x] = src[(long)j * ld + x];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += blockDim.y) {
        const int x = bx + r, j = by + threadIdx.x;
        if (x < W && j < ny) dst[(long)(i0 + x) * pitch + j] = half_store(tile[threadIdx.x][r], w);
    }
}

// "The last block of a member finishes the sum": called by every thread of a block once the block's partials of member m are
// written.  tickets[m * STRIDE] counts the member's blocks that have got here in this launch (0 between launches), nblocks is
// how many there are.  Block-uniform; true in exactly one block per member and launch, the one that drew the last ticket, which
// may then read all the member's partials through a volatile pointer, because
//  * the first barrier (SYNC) puts the stores of all the block's threads before thread 0's fence.  SYNC = false is for a
//    block whose only partial thread 0 wrote itself (forces_block): program order does the same;
//  * thread 0's __threadfence() makes those stores visible device-wide before its atomicAdd counts the block, so the block
//    that reads nblocks - 1 there does so after the partials of all the others became visible;
//  * the second barrier hands thread 0's verdict to the block, and the second fence, with the volatile pointer, keeps the
//    reads that follow from being served by anything fetched before the ticket was drawn.
// The ticket is left as it is: the thread that writes the member's result zeroes it, for the next launch in the stream.
template <bool SYNC, int STRIDE>
__device__ __forceinline__ bool member_done(unsigned int *tickets, long m, unsigned int nblocks)
{
    __shared__ int last;
    if (SYNC) __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(&tickets[m * STRIDE], 1u) == nblocks - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    return true;
}

// wt_forces of every member in one launch: grid (nb, B).  Each block computes k_forces' partial of its block index; the
// member's last block (member_done) sums its nb partials in block order, in double, as wt_forces does on the host, and
// writes one row entry.
template <typename T>
__global__ __launch_bounds__(256) void k_forces_batch(const T *__restrict__ macro, const uint8_t *__restrict__ mask, Geom g,
                                                      MemberStrides ms, int nb, ForcePartial *__restrict__ part,
                                                      unsigned int *__restrict__ tickets, double *__restrict__ fx,
                                                      double *__restrict__ fy, long long *__restrict__ surf,
                                                      long long *__restrict__ rev)
{
    const long m = blockIdx.y;
    ForcePartial *p = part + m * nb;
    forces_block<T>(macro + m * ms.macro, mask + m * ms.mask, g, 0, g.nxl, (int)blockIdx.x, nb, p + blockIdx.x);
    if (!member_done<false, 1>(tickets, m, (unsigned)nb) || threadIdx.x != 0) return;      // (adjacent tickets)
    const volatile ForcePartial *vp = p;
    double sx = 0.0, sy = 0.0;
    long long ns = 0, nr = 0;
    for (int b = 0; b < nb; b++) { sx += vp[b].fx; sy += vp[b].fy; ns += vp[b].surf; nr += vp[b].rev; }
    fx[m] = sx; fy[m] = sy; surf[m] = ns; rev[m] = nr;
    tickets[m] = 0;
}

// Surface loads of every member in one launch: grid (ceil(NX / kLoadsWaves), B), one wave per (member, column i).  The time
// of the launch follows its number of blocks (one device-wide fence and one ticket each), hence the large blocks.  A column is one
// contiguous run of the mask and of rho (y fastest), read in chunks of 64 rows, one row per lane; rows past NY never count.
//  * Moment: forces_block's faces (fluid cell, solid 4-neighbour inside the grid in direction d, p = (double)rho / 3, force
//    p * d at the face centre r = (i + 0.5 + 0.5 dx, j + 0.5 + 0.5 dy)), each adding (r.x - xr) F.y - (r.y - yr) F.x.  The
//    column's terms are added by wave_sum; the member's last block (member_done) adds the columns' partials in column order.
//  * Surface: the highest and lowest solid row of the column from the chunks' ballots; with `accumulate`, rho of the fluid
//    cell above the one and below the other is added to the member's sums.  One lane owns an entry and launches are
//    stream-ordered, so the sums are plain read-modify-writes in sample order.
template <typename T>
__global__ __launch_bounds__(kLoadsWaves * 64) void k_loads_batch(const T *__restrict__ macro, const uint8_t *__restrict__ mask, Geom g,
                                                     MemberStrides ms, const double *__restrict__ ref, double *__restrict__ col,
                                                     unsigned int *__restrict__ tickets, double *__restrict__ mz,
                                                     double *__restrict__ s_rho, long long *__restrict__ s_cnt, int accumulate)
{
    const long m = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int nx = g.nxl, ny = g.ny;
    const int i = (int)blockIdx.x * kLoadsWaves + (int)(threadIdx.x >> 6);
    if (i < nx) {                                                   // (wave-uniform)
        const uint8_t *mk = mask + m * ms.mask + g.pitch + (long)i * g.pitch;      // column i of the padded mask
        const T *rho = macro + m * ms.macro + (long)i * g.pitch;
        const double xr = ref[2 * m], yr = ref[2 * m + 1];
        const double ax = ((double)i + 0.5) - xr;                   // r.x - xr of the column's horizontal faces
        const bool left = i > 0, right = i + 1 < nx;
        double t = 0.0;
        int jhi = -1, jlo = ny;
        for (int j0 = 0; j0 < ny; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j < ny;
            const int solid = in && mk[j];
            const unsigned long long sb = __ballot(solid);
            if (sb) {
                jhi = j0 + 63 - __clzll((long long)sb);
                if (jlo == ny) jlo = j0 + __ffsll((unsigned long long)sb) - 1;
            }
            if (in && !solid) {
                const int sxp = right && mk[g.pitch + j];
                const int sxm = left && mk[j - g.pitch];
                const int syp = (j + 1 < ny) && mk[j + 1];
                const int sym = (j > 0) && mk[j - 1];
                if (sxp + sxm + syp + sym) {
                    const double p = (double)rho[j] / 3.0;
                    const double ay = ((double)j + 0.5) - yr;       // r.y - yr of the cell's vertical faces
                    if (sxp) t -= ay * p;                           // F = (+p, 0) at (i + 1, j + 0.5)
                    if (sxm) t += ay * p;                           // F = (-p, 0) at (i, j + 0.5)
                    if (syp) t += ax * p;                           // F = (0, +p) at (i + 0.5, j + 1)
                    if (sym) t -= ax * p;                           // F = (0, -p) at (i + 0.5, j)
                }
            }
        }
        t = wave_sum(t);
        if (lane == 0) {
            col[m * nx + i] = t;
            if (accumulate) {
                const long e = (m * 2) * nx + i;                    // upper; the lower entry is nx further on
                if (jhi >= 0 && jhi + 1 < ny) { s_rho[e] += (double)rho[jhi + 1]; s_cnt[e] += 1; }
                if (jlo < ny && jlo > 0) { s_rho[e + nx] += (double)rho[jlo - 1]; s_cnt[e + nx] += 1; }
            }
        }
    }
    constexpr int NT = kLoadsWaves * 64;
    __shared__ double sh[NT];
    if (!member_done<true, kTicketStride>(tickets, m, gridDim.x)) return;
    const volatile double *vc = col + m * nx;
    double s = 0.0;
    for (int c0 = 0; c0 < nx; c0 += NT) {                           // NT partials at a time through LDS; thread 0 adds them in column order
        const int c = c0 + (int)threadIdx.x;
        sh[threadIdx.x] = c < nx ? vc[c] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = nx - c0 < NT ? nx - c0 : NT;
            for (int k = 0; k < n; k++) s += sh[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { mz[m] = s; tickets[m * kTicketStride] = 0; }
}

// Momentum exchange of every member in one launch: grid (ceil(W / kLoadsWaves), B), one wave per (member, column), W the widest
// member's window.  Definition (include/wt_polar.h): directions e_k, k = 1..8, as d2q9.hpp / html:238-248; cell (i, j) covers
// [i, i+1) x [j, j+1).  After step n the current lattice holds, in every interior fluid cell x (not solid, 1 <= i <= NX-2,
// 1 <= j <= NY-2: the cells that take STEP_FS's interior branch), the post-collision populations f*_k(x, n).  A link is a pair
// (interior fluid cell x, direction k) whose neighbour x + e_k is solid.  In step n+1 the population f*_k(x, n) that leaves x
// along the link comes back to x as population opp(k) unchanged (half-way bounce-back), so the body receives the momentum
// 2 f*_k(x, n) e_k per step from that link.  Hence, all in double from the stored values converted exactly:
//   F = sum over the links of 2 (double)f*_k(x) e_k (diagonal links included),
//   Mz = sum over the links of (r.x - xref) F_link.y - (r.y - yref) F_link.x, r = (i + 0.5 + 0.5 e_kx, j + 0.5 + 0.5 e_ky),
//   links = the number of links.
// No rest-state term is subtracted; boundary cells own no link.
// A member's window win[m] = (first column, columns) holds every interior column next to one of its solid columns: no other
// column can own a link.  A column is one contiguous run of the mask and of each population plane (y fastest), read in chunks of
// 64 rows, one row per lane: the mask bytes of columns i-1, i, i+1 at rows j-1, j, j+1, then a population only on the lanes that
// own a link in its direction.  The column's terms are added by wave_sum; the member's last block (member_done) adds the
// columns' partials in column order, each of the four sums on a wave of its own.
// E is the lattice's stored element.  `link(fc, mk, g, m, coloff, j, k, t, q)` is the link rule: for the link of direction k that the cell
// at row j of the column owns (fc and mk the column in population plane 0 and in the mask, coloff its offset in a padded plane), t is
// the magnitude of the momentum the link hands over, so that F_link = t e_k, and q the distance from the cell's centre to the link's
// point, r = (i + 0.5 + q e_kx, j + 0.5 + q e_ky), both doubles.  The definition above is the half-way rule, t = 2 f*_k(x) and q = 0.5.
template <typename E, typename Link>
__device__ __forceinline__ void mex_member(const E *__restrict__ f, const uint8_t *__restrict__ mask, const Geom &g, const MemberStrides &ms,
                                           const double *__restrict__ ref, const int32_t *__restrict__ win, MexPartial *__restrict__ col,
                                           unsigned int *__restrict__ tickets, double *__restrict__ fx, double *__restrict__ fy,
                                           double *__restrict__ mz, long long *__restrict__ links, const Link &link)
{
    const long m = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int nx = g.nxl, ny = g.ny;
    const int width = win[2 * m + 1];
    const int c = (int)blockIdx.x * kLoadsWaves + (int)(threadIdx.x >> 6);
    if (c < width) {                                                // (wave-uniform)
        const int i = win[2 * m] + c;                               // 1 <= i <= NX-2 (mex_window)
        const long coloff = g.pitch + (long)i * g.pitch;            // column i of a padded plane
        const uint8_t *mk = mask + m * ms.mask + coloff;            // ... of the mask
        const E *fc = f + m * ms.lat + coloff;                      // ... of population plane 0
        const double xr = ref[2 * m], yr = ref[2 * m + 1];
        double sx = 0.0, sy = 0.0, sm = 0.0;
        long long n = 0;
        for (int j0 = 0; j0 < ny; j0 += 64) {
            const int j = j0 + lane;
            unsigned s = 0;                                         // bit k: this lane's cell owns a link in direction k
            if (j >= 1 && j <= ny - 2 && !mk[j]) {
                const uint8_t *l = mk - g.pitch + j, *r = mk + g.pitch + j;
                s = (r[0] ? 1u << 1 : 0u) | (mk[j + 1] ? 1u << 2 : 0u) | (l[0] ? 1u << 3 : 0u) | (mk[j - 1] ? 1u << 4 : 0u) |
                    (r[1] ? 1u << 5 : 0u) | (l[1] ? 1u << 6 : 0u) | (l[-1] ? 1u << 7 : 0u) | (r[-1] ? 1u << 8 : 0u);
            }
            if (__ballot(s != 0) == 0ULL) continue;
#pragma unroll
            for (int k = 1; k <= 8; k++) {
                if (!(s >> k & 1u)) continue;
                double t, q;                                        // the link's magnitude and its distance to the wall
                link(fc, mk, g, m, coloff, j, k, t, q);
                const double flx = t * (double)ex_of(k), fly = t * (double)ey_of(k);
                const double rx = ((double)i + 0.5) + q * (double)ex_of(k), ry = ((double)j + 0.5) + q * (double)ey_of(k);
                const double a = (rx - xr) * fly, b = (ry - yr) * flx;
                sx += flx;
                sy += fly;
                sm += a - b;
                n += 1;
            }
        }
        sx = wave_sum(sx); sy = wave_sum(sy); sm = wave_sum(sm); n = wave_sum(n);
        if (lane == 0) {
            MexPartial p;
            p.fx = sx; p.fy = sy; p.mz = sm; p.links = n;
            col[m * nx + c] = p;
        }
    }
    constexpr int NT = kLoadsWaves * 64;
    __shared__ double sh[3][NT];
    __shared__ long long shn[NT];
    if (!member_done<true, kTicketStride>(tickets, m, gridDim.x)) return;
    const volatile MexPartial *vc = col + m * nx;
    const int w = (int)(threadIdx.x >> 6);
    double s = 0.0;                                                 // lane 0 of wave 0, 1, 2: Fx, Fy, Mz
    long long sn = 0;                                               // lane 0 of wave 3: links
    for (int c0 = 0; c0 < width; c0 += NT) {                        // NT partials at a time through LDS, added in column order
        const int p = c0 + (int)threadIdx.x;
        const bool in = p < width;
        sh[0][threadIdx.x] = in ? vc[p].fx : 0.0;
        sh[1][threadIdx.x] = in ? vc[p].fy : 0.0;
        sh[2][threadIdx.x] = in ? vc[p].mz : 0.0;
        shn[threadIdx.x] = in ? vc[p].links : 0;
        __syncthreads();
        if (lane == 0 && w < 4) {
            const int cnt = width - c0 < NT ? width - c0 : NT;
            if (w < 3) for (int k = 0; k < cnt; k++) s += sh[w][k];
            else for (int k = 0; k < cnt; k++) sn += shn[k];
        }
        __syncthreads();
    }
    if (lane == 0) {
        if (w == 0) { fx[m] = s; tickets[m * kTicketStride] = 0; }
        else if (w == 1) fy[m] = s;
        else if (w == 2) mz[m] = s;
        else if (w == 3) links[m] = sn;
    }
}

// The half-way link: t = 2 f*_k(x), f*_k(x) the stored population through Load (lat_load: the identity for a native lattice,
// (float)h + w_k for a half batch) converted exactly to double, and q = 0.5.
template <typename T>
struct LinkHalfway {
    template <typename E>
    __device__ __forceinline__ void operator()(const E *__restrict__ fc, const uint8_t *__restrict__, const Geom &g, long, long, int j, int k,
                                               double &t, double &q) const
    {
        t = 2.0 * (double)lat_load<T>(fc + k * g.plane + j, k);
        q = 0.5;
    }
};

// The interpolated link (include/wt_polar.h "Interpolated bounce-back"): t = (double)a + (double)b, a = f*_k(x) and b the value the next
// step will reflect (wall_incoming of the current lattice, in T), and q the link's wall distance converted exactly, so that the link's
// point is the wall point.  wq holds the members' wall distances (eight planes each, laid out like population planes 1..8, qstride
// elements apart), read, like the populations, only on the lanes that own a link.  At q = 0.5 both are the half-way link's.
template <typename T>
struct LinkInterp {
    const T *__restrict__ wq;
    long qstride;
    __device__ __forceinline__ void operator()(const T *__restrict__ fc, const uint8_t *__restrict__ mk, const Geom &g, long m, long coloff, int j,
                                               int k, double &t, double &q) const
    {
        const long back = j - ey_of(k) - (long)ex_of(k) * g.pitch;      // x - e_k, from column i
        const T qk = wq[m * qstride + coloff + (k - 1) * g.plane + j], fa = fc[k * g.plane + j];
        const T fb = wall_incoming<T>(qk, fa, fc + k * g.plane + back, mk[back] != 0, fc + opp_of(k) * g.plane + j);
        t = (double)fa + (double)fb;
        q = (double)qk;
    }
};

// The moving-wall link (include/wt_polar.h "Wall velocity"): LinkInterp with b from the moving-wall overload of wall_incoming and the link's
// wall-normal velocity, read from wu (laid out like wq, ustride elements between members) on the lanes that own the link.  With +0 in every
// entry it is LinkInterp's.
template <typename T>
struct LinkMoving {
    const T *__restrict__ wq;
    long qstride;
    const T *__restrict__ wu;
    long ustride;
    __device__ __forceinline__ void operator()(const T *__restrict__ fc, const uint8_t *__restrict__ mk, const Geom &g, long m, long coloff, int j,
                                               int k, double &t, double &q) const
    {
        const long back = j - ey_of(k) - (long)ex_of(k) * g.pitch;      // x - e_k, from column i
        const long e = coloff + (k - 1) * g.plane + j;
        const T qk = wq[m * qstride + e], un = wu[m * ustride + e], fa = fc[k * g.plane + j];
        const T fb = wall_incoming<T>(qk, fa, fc + k * g.plane + back, mk[back] != 0, fc + opp_of(k) * g.plane + j, link_weight<T>(k), un);
        t = (double)fa + (double)fb;
        q = (double)qk;
    }
};

// The kernel of the momentum exchange: mex_member with the link rule as an argument, by value, with what the rule reads per member.  Every
// (E, Link) is a kernel of its own, so that a batch runs the one its storage and wall rule select (launch_mex) and no other.  ms.lat counts
// the lattice's elements: T, or halves.
template <typename E, typename Link>
__global__ __launch_bounds__(kLoadsWaves * 64) void k_mex_batch(const E *__restrict__ f, const uint8_t *__restrict__ mask, Geom g,
                                                   MemberStrides ms, const double *__restrict__ ref, const int32_t *__restrict__ win,
                                                   MexPartial *__restrict__ col, unsigned int *__restrict__ tickets,
                                                   double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ mz,
                                                   long long *__restrict__ links, Link link)
{
    mex_member(f, mask, g, ms, ref, win, col, tickets, fx, fy, mz, links, link);
}

// Every element of p[0, n) set to v: the wall distances' default.
template <typename T>
__global__ __launch_bounds__(256) void k_fill_value(T *__restrict__ p, long n, T v)
{
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x) p[t] = v;
}

// Mean fields of every member in one launch: grid (ceil(NX * ceil(NY / R) / 256), B), R = WTP_MEAN_ROWS; one lane per run of R
// consecutive rows of one column.  Definition (include/wt_polar.h): for member m and cell (i, j), let rho, ux, uy be what
// wtp_read_macro would return after a sampled step, converted exactly to double.  Solid and boundary cells are included; no cell
// is special-cased.  The device keeps seven running sums per cell, in double, added in sample order: sum rho, sum ux, sum uy,
// sum rho*rho, sum ux*ux, sum uy*uy, sum ux*uy.  Each product is one double multiplication, added as a separate operation;
// nothing is fused.  For fp32 members the products are exact in double; for fp64 members they round once, as NumPy's do.  In
// both cases the seven sums are bit-identical to a NumPy loop over wtp_read_macro at the sampled steps.  The device also keeps a
// per-member sample count n (int64).
// A pure stream: a lane loads its run of each of the three emitted planes ([NX][pitch], y fastest) and of each of the seven sum
// planes ([NX][apitch], apitch = NY rounded up to R, so that rows past NY are never moved), adds, and stores the seven runs
// back.  Every entry has one owner and launches are stream-ordered: plain read-modify-writes in sample order.  With R = 2 a lane
// moves 16 bytes per access to the sums and 8 or 16 per access to the fields.  A run that starts at row NY - 1 of an odd NY owns
// one row; its second field element lies in the column's pad (pitch > NY there) and is loaded, not used.
template <typename T>
__global__ __launch_bounds__(256) void k_mean_batch(const T *__restrict__ macro, Geom g, MemberStrides ms, double *__restrict__ sums,
                                                    long stride, int apitch, long long *__restrict__ count)
{
    constexpr int R = WTP_MEAN_ROWS;
    const long m = blockIdx.y;
    const int nx = g.nxl, ny = g.ny;
    const int runs = (ny + R - 1) / R;                              // runs of a column
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q == 0) count[m] += 1;
    if (q >= (long)nx * runs) return;
    const int i = (int)(q / runs), j = (int)(q - (long)i * runs) * R;
    const long mp = (long)nx * g.pitch, ap = (long)nx * apitch;     // elements of one field plane / one sum plane
    const T *src = macro + m * ms.macro + (long)i * g.pitch + j;
    double *acc = sums + m * stride + (long)i * apitch + j;
    RowRun<T, R> fld[3];
    RowRun<double, R> s[kMeanPlanes];
#pragma unroll
    for (int a = 0; a < 3; a++) fld[a] = *reinterpret_cast<const RowRun<T, R> *>(src + a * mp);
#pragma unroll
    for (int k = 0; k < kMeanPlanes; k++) s[k] = *reinterpret_cast<const RowRun<double, R> *>(acc + k * ap);
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (j + r >= ny) continue;
        const double rho = (double)fld[0][r], ux = (double)fld[1][r], uy = (double)fld[2][r];
        const double rr = rho * rho, uu = ux * ux, vv = uy * uy, uv = ux * uy;
        s[0][r] += rho; s[1][r] += ux; s[2][r] += uy;
        s[3][r] += rr; s[4][r] += uu; s[5][r] += vv; s[6][r] += uv;
    }
#pragma unroll
    for (int k = 0; k < kMeanPlanes; k++) *reinterpret_cast<RowRun<double, R> *>(acc + k * ap) = s[k];
}

// Probe points of every member in one launch: grid (ceil(P / 256), members), blockIdx.y the member, one lane per point.  Definition
// (include/wt_polar.h "Probe points"): member m holds P points; point p has a base cell (i0, j0), held as its offset off = i0 * pitch + j0
// in a macroscopic plane ([NX][pitch], y fastest; -1 flags an inactive point), and four weights w00, w10, w01, w11 for the cells (i0, j0),
// (i0+1, j0), (i0, j0+1), (i0+1, j0+1), all formed and checked on the host (probe_tables), so that every offset read here lies inside the
// member's planes: i0 <= NX - 2 and j0 <= NY - 2.  For each of the three planes a in (rho, ux, uy), with the four values converted exactly
// to double:
//     v = ((w00*a00 + w10*a10) + w01*a01) + w11*a11
// with no contraction (the file is built with -ffp-contract=off): seven roundings.  No cell is special-cased.
// The tables are structure of arrays per member (off [P], w [4][P]), so that consecutive lanes read consecutive entries; the twelve gathers
// of a lane fall into two neighbouring columns of each plane.  ACCUMULATE: the three values are added to the point's sums, out[a][p] += v,
// and lane 0 of block 0 adds one to the member's count, as k_mean_batch does; every entry has one owner and launches are stream-ordered, so
// these are plain read-modify-writes in sample order, with no atomics and no tickets, and an inactive point does nothing.  Without
// ACCUMULATE the three values go to out[a][p] (the scratch row of wtp_probe_sample), NaN at an inactive point, and count is not touched.
// macro, off, w, out and count are those of member blockIdx.y = 0: the on-demand call hands in one member's with a grid of one row.
template <typename T, bool ACCUMULATE>
__global__ __launch_bounds__(256) void k_probe_batch(const T *__restrict__ macro, Geom g, MemberStrides ms, int npoints,
                                                     const long long *__restrict__ off, const double *__restrict__ w,
                                                     double *__restrict__ out, long long *__restrict__ count)
{
    const long m = blockIdx.y;
    const long P = npoints;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (ACCUMULATE && p == 0) count[m] += 1;
    if (p >= P) return;
    double *dst = out + m * 3 * P + p;
    const long long o = off[m * P + p];
    if (o < 0) {
        if (!ACCUMULATE) { dst[0] = __builtin_nan(""); dst[P] = __builtin_nan(""); dst[2 * P] = __builtin_nan(""); }
        return;
    }
    const double *wm = w + m * 4 * P + p;
    const double w00 = wm[0], w10 = wm[P], w01 = wm[2 * P], w11 = wm[3 * P];
    const long mp = (long)g.nxl * g.pitch;                          // elements of one field plane
    const T *src = macro + m * ms.macro + o;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const T *s = src + a * mp;
        const double a00 = (double)s[0], a10 = (double)s[g.pitch], a01 = (double)s[1], a11 = (double)s[g.pitch + 1];
        const double v = ((w00 * a00 + w10 * a10) + w01 * a01) + w11 * a11;
        if (ACCUMULATE) dst[a * P] += v;
        else dst[a * P] = v;
    }
}

// The device-side far-field vortex (include/wt_polar.h "Device-side far-field vortex") of every member in one launch, behind
// k_forces_batch: grid (ceil((NY + 2 NX) / kVortexBlock), B), blockIdx.y the member, one lane per table entry, the entries in the order
// left[0 .. NY), bottom[0 .. NX), top[0 .. NX), so that consecutive lanes write consecutive entries of a table plane.  Definition, all in
// double, one rounding per operation, left to right as written, no contraction, IEEE division and square root:
//   Update (UPDATE only) of member m from (fx, fy), wtp_forces' values of the last emitted state, with c = cos_a[m], s = sin_a[m]:
//     drag = fx*c + fy*s;   lift = (-fx)*s + fy*c
//     ts   = lift/den;      tq = with_source ? drag/den : 0.0
//     ns   = strength + relax*(ts - strength);   nq = source + relax*(tq - source)
//     speed   = sqrt(ns*ns + nq*nq)/bound
//     clipped = speed > 0.1;   scale = clipped ? 0.1/speed : 1.0
//     strength = ns*scale;  source = nq*scale
//   Tables, for the cell (i, j) of an entry (left: (0, j); bottom: (i, 0); top: (i, NY-1)), each value rounded to T once:
//     dx = i + 0.5 - xc;  dy = j + 0.5 - yc;  r2 = dx*dx + dy*dy
//     ux = u_far + strength*dy/r2 + source*dx/r2
//     uy = v_far - strength*dx/r2 + source*dy/r2
//     rho = 1 + 1.5*((u_far*u_far + v_far*v_far) - (ux*ux + uy*uy))
// The update is scalar work that every lane repeats for its member: the same operations on the same inputs, the same bits in every
// block, so that no block waits for another.  The strengths are double-buffered by update parity: every block reads the pair of
// `cur`, which an earlier launch wrote, and block 0 of the member alone writes the new pair to `next` and the log row, so no block
// reads what another replaces.  No atomics, no fence.  Without UPDATE the tables are built from `cur` as it is (wtp_enable_far_vortex,
// wtp_set_far_vortex) and fx, fy, next and the log are not touched.  member: [4][B] u_far, v_far, cos_a, sin_a; cur, next: [2][B]
// strength, source; log: row r of column c (fx, fy, strength, source) at log[c * log_col + m]; clip[m].  Entries past NY of `left` and
// past NX of `bottom` and `top` are not written and keep their +0.
template <typename T, bool UPDATE>
__global__ __launch_bounds__(kVortexBlock) void k_far_vortex(T *__restrict__ prof, long pstride, long pitch, int nxp, int nx, int ny, VortexSet v,
                                                             const double *__restrict__ member, const double *__restrict__ fx,
                                                             const double *__restrict__ fy, const double *__restrict__ cur,
                                                             double *__restrict__ next, double *__restrict__ log, long log_col,
                                                             int32_t *__restrict__ clip)
{
    const long m = blockIdx.y, B = gridDim.y;
    const double u_far = member[m], v_far = member[B + m];
    double strength = cur[m], source = cur[B + m];
    if (UPDATE) {
        const double c = member[2 * B + m], s = member[3 * B + m];
        const double f_x = fx[m], f_y = fy[m];
        const double drag = f_x * c + f_y * s, lift = (-f_x) * s + f_y * c;
        const double ts = lift / v.den, tq = v.with_source ? drag / v.den : 0.0;
        const double ns = strength + v.relax * (ts - strength), nq = source + v.relax * (tq - source);
        const double speed = sqrt(ns * ns + nq * nq) / v.bound;
        const bool clipped = speed > 0.1;
        const double scale = clipped ? 0.1 / speed : 1.0;
        strength = ns * scale;
        source = nq * scale;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            next[m] = strength; next[B + m] = source;
            log[m] = f_x; log[log_col + m] = f_y; log[2 * log_col + m] = strength; log[3 * log_col + m] = source;
            clip[m] = clipped ? 1 : 0;
        }
    }
    int e = (int)blockIdx.x * kVortexBlock + (int)threadIdx.x;     // the entry: left, then bottom, then top
    T *tab = prof + m * pstride;
    long ps = pitch;                                                // elements between the planes of the entry's table
    int i = 0, j = e;
    if (e >= ny) {
        e -= ny;
        if (e >= 2 * nx) return;
        const bool top = e >= nx;
        if (top) e -= nx;
        tab += 3 * pitch + (top ? 3 * (long)nxp : 0);
        ps = nxp;
        i = e; j = top ? ny - 1 : 0;
    }
    const double dx = ((double)i + 0.5) - v.xc, dy = ((double)j + 0.5) - v.yc;
    const double r2 = dx * dx + dy * dy;
    const double ux = (u_far + strength * dy / r2) + source * dx / r2;
    const double uy = (v_far - strength * dx / r2) + source * dy / r2;
    const double rho = 1.0 + 1.5 * ((u_far * u_far + v_far * v_far) - (ux * ux + uy * uy));
    tab[e] = (T)rho; tab[ps + e] = (T)ux; tab[2 * ps + e] = (T)uy;
}

// ------------------------------------------------------------------------------------------
// life cycle
// ------------------------------------------------------------------------------------------
template <typename T> static T *fptr(wtp_batch *b, int which, int m) { return reinterpret_cast<T *>(b->f[which]) + (long)m * b->ms.lat; }
template <typename T> static T *macro_of(wtp_batch *b, int m) { return reinterpret_cast<T *>(b->macro) + (long)m * b->ms.macro; }

static int check_batch(const wtp_batch *b)
{
    if (!b) return fail(WT_ERR_ARG, "null batch");
    return WT_OK;
}

static int check_members(const wtp_batch *b, int first, int count)
{
    if (first < 0 || count < 1 || first + count > b->members)
        return fail(WT_ERR_ARG, "members [%d, %d) outside the batch of %d", first, first + count, b->members);
    return WT_OK;
}

static int check_member(const wtp_batch *b, int member)
{
    if (member < 0 || member >= b->members) return fail(WT_ERR_ARG, "member %d outside the batch of %d", member, b->members);
    return WT_OK;
}

// What a half batch does not have: `what` names it.
static int check_native(const wtp_batch *b, const char *what)
{
    if (b->storage == WTP_STORE_HALF) return fail(WT_ERR_STATE, "%s is not available in a half batch", what);
    return WT_OK;
}

// f(T()) with T the batch's dtype, float or double: the run-time dtype handed on as a type (decltype of f's argument).
template <typename F>
static auto with_dtype(const wtp_batch *b, F f)
{
    return b->dtype == WT_F32 ? f(float()) : f(double());
}

static int ensure_stage(wtp_batch *b, size_t bytes)
{
    if (b->stage_bytes >= bytes) return WT_OK;
    if (b->stage) { HIP_TRY(hipFree(b->stage)); b->stage = nullptr; b->stage_bytes = 0; }
    WT_TRY(alloc_all({{&b->stage, bytes}}, "stage"));
    b->stage_bytes = bytes;
    return WT_OK;
}

extern "C" int wtp_destroy(wtp_batch *b)
{
    if (!b) return WT_OK;
    (void)hipSetDevice(b->device);
    if (b->st) (void)hipStreamSynchronize(b->st);
    void *bufs[] = {b->f[0], b->f[1], b->macro, b->mask, b->tiles, b->params, b->les_c, b->wq, b->wu, b->wind_v, b->trt_lam, b->zero_v, b->prof, b->v_member, b->v_str, b->v_forces, b->v_log, b->v_clip, b->partials, b->tickets, b->stage,
                    b->l_ref, b->l_col, b->l_tickets, b->s_rho, b->s_cnt, b->x_win, b->x_ref, b->x_col, b->x_tickets, b->m_sums, b->m_cnt,
                    b->pb_off, b->pb_w, b->pb_sums, b->pb_cnt, b->pb_row};
    for (void *p : bufs) if (p) (void)hipFree(p);
    for (SampleTable *t : {&b->forces, &b->moment, &b->xforces}) t->release();
    if (b->st) (void)hipStreamDestroy(b->st);
    delete b;
    return WT_OK;
}

extern "C" int wtp_create(int nx, int ny, int dtype, int members, int history_cap, int device, wtp_batch **out)
{
    return wtp_create_stored(nx, ny, dtype, WTP_STORE_NATIVE, members, history_cap, device, out);
}

extern "C" int wtp_create_stored(int nx, int ny, int dtype, int storage, int members, int history_cap, int device, wtp_batch **out)
{
    if (!out) return fail(WT_ERR_ARG, "out is null");
    *out = nullptr;
    if (nx < 3 || ny < 3) return fail(WT_ERR_ARG, "lattice must be at least 3x3 (got %dx%d)", nx, ny);
    if ((long long)nx * ny > (1LL << 33)) return fail(WT_ERR_ARG, "lattice too large");
    if (dtype != WT_F32 && dtype != WT_F64) return fail(WT_ERR_ARG, "dtype must be WT_F32 or WT_F64");
    if (storage != WTP_STORE_NATIVE && storage != WTP_STORE_HALF)
        return fail(WT_ERR_ARG, "storage must be WTP_STORE_NATIVE or WTP_STORE_HALF (got %d)", storage);
    if (storage == WTP_STORE_HALF && dtype != WT_F32) return fail(WT_ERR_ARG, "storage WTP_STORE_HALF needs dtype WT_F32");
    if (members < 1 || members > WTP_MAX_MEMBERS) return fail(WT_ERR_ARG, "members must be in [1, %d] (got %d)", WTP_MAX_MEMBERS, members);
    if (history_cap < 0) return fail(WT_ERR_ARG, "history_cap must be >= 0 (got %d)", history_cap);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(WT_ERR_HIP, "no HIP device available (%s); libwtpolar has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(WT_ERR_ARG, "device %d out of range (0..%d)", device, ndev - 1);
    HIP_TRY(hipSetDevice(device));

    wtp_batch *b = new (std::nothrow) wtp_batch();
    if (!b) return fail(WT_ERR_OOM, "host allocation failed");
    b->nx = nx; b->ny = ny; b->dtype = dtype; b->device = device; b->members = members; b->cap = history_cap;
    b->esz = dtype == WT_F32 ? 4 : 8;
    b->storage = storage;
    b->lat_esz = storage == WTP_STORE_HALF ? 2 : b->esz;
    Geom &g = b->g;                              // wt_create's geometry of a whole lattice
    g.nxl = nx; g.ny = ny; g.gi0 = 0; g.nx_g = nx;
    g.pitch = ((long)ny + 255) / 256 * 256;
    g.plane = (((long)(g.nxl + 2) * g.pitch * (long)b->esz + 4095) / 4096 * 4096 + 17408) / (long)b->esz;
    b->tiles_per_col = (int)(g.pitch / tile_j_of(b->esz));
    b->ms.lat = member_stride((size_t)9 * g.plane * b->lat_esz, b->lat_esz);      // (a half batch keeps pitch and plane, in 2-byte elements)
    b->ms.macro = member_stride((size_t)3 * g.nxl * g.pitch * b->esz, b->esz);
    b->ms.mask = member_stride((size_t)(g.nxl + 2) * g.pitch, 1);
    b->ms.tiles = member_stride((size_t)g.nxl * b->tiles_per_col, 1);
    b->nb = reduce_blocks((long)nx * ny);
    b->mask_set.assign((size_t)members, 0);
    b->surf_rows.assign((size_t)members * 2 * nx, -1);
    b->mex_win.assign((size_t)members * 2, 0);

    auto cleanup = [&](int rc) { wtp_destroy(b); return rc; };
#define CREATE_TRY(expr)                                                                               \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return cleanup(fail(e_ == hipErrorOutOfMemory ? WT_ERR_OOM : WT_ERR_HIP, "%s failed: %s",  \
                                #expr, hipGetErrorString(e_)));                                        \
    } while (0)
    const size_t B = (size_t)members;
    const size_t lat_bytes = B * b->ms.lat * b->lat_esz, macro_bytes = B * b->ms.macro * b->esz;
    const size_t mask_bytes = B * b->ms.mask, tile_bytes = B * b->ms.tiles;
    CREATE_TRY(hipStreamCreateWithFlags(&b->st, hipStreamNonBlocking));
    CREATE_TRY(hipMalloc(&b->f[0], lat_bytes));
    CREATE_TRY(hipMalloc(&b->f[1], lat_bytes));
    CREATE_TRY(hipMalloc(&b->macro, macro_bytes));
    CREATE_TRY(hipMalloc((void **)&b->mask, mask_bytes));
    CREATE_TRY(hipMalloc((void **)&b->tiles, tile_bytes));
    CREATE_TRY(hipMalloc(&b->params, B * 2 * b->esz));
    CREATE_TRY(hipMalloc((void **)&b->partials, B * b->nb * sizeof(ForcePartial)));
    CREATE_TRY(hipMalloc((void **)&b->tickets, B * sizeof(unsigned int)));
    if (int rc = b->forces.alloc(4, (size_t)history_cap, B, "force history")) return cleanup(rc);
    CREATE_TRY(hipMemsetAsync(b->f[0], 0, lat_bytes, b->st));
    CREATE_TRY(hipMemsetAsync(b->f[1], 0, lat_bytes, b->st));
    CREATE_TRY(hipMemsetAsync(b->macro, 0, macro_bytes, b->st));
    CREATE_TRY(hipMemsetAsync(b->mask, 0, mask_bytes, b->st));
    CREATE_TRY(hipMemsetAsync(b->tiles, 0, tile_bytes, b->st));
    CREATE_TRY(hipMemsetAsync(b->tickets, 0, B * sizeof(unsigned int), b->st));
    CREATE_TRY(hipStreamSynchronize(b->st));
#undef CREATE_TRY
    *out = b;
    return WT_OK;
}

extern "C" const char *wtp_last_error(void) { return g_err; }

extern "C" const char *wtp_version(void) { return "libwtpolar 0.4 (gfx950, batched D2Q9 members, column-major SoA, surface loads, momentum exchange, mean fields, Smagorinsky subgrid viscosity, interpolated bounce-back, inclined free stream, half-precision population storage, state upload and restart, two-relaxation-time collision, prescribed far-field profile, device-side far-field vortex, probe points, wall velocity)"; }

extern "C" int wtp_sync(wtp_batch *b)
{
    WT_TRY(check_batch(b));
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// masks and state
// ------------------------------------------------------------------------------------------
// Rows of the fluid cells directly above the highest / below the lowest solid cell of every column of one [NY][NX] mask;
// -1 where the column holds no solid cell or its extreme one touches the border.
static void surface_rows(wtp_batch *b, int member, const uint8_t *m01)
{
    const int nx = b->nx, ny = b->ny;
    int32_t *up = b->surf_rows.data() + (size_t)member * 2 * nx, *lo = up + nx;
    for (int i = 0; i < nx; i++) {
        int jhi = -1, jlo = ny;
        for (int j = 0; j < ny; j++)
            if (m01[(size_t)j * nx + i]) { jhi = j; if (jlo == ny) jlo = j; }
        up[i] = (jhi >= 0 && jhi + 1 < ny) ? jhi + 1 : -1;
        lo[i] = (jlo < ny && jlo > 0) ? jlo - 1 : -1;
    }
}

// The columns of one [NY][NX] mask that can own a momentum-exchange link: the interior columns (1 .. NX-2) from the one before
// its first solid column to the one after its last.  (first column, count); count 0 where the mask holds no solid cell.
static void mex_window(wtp_batch *b, int member, const uint8_t *m01)
{
    const int nx = b->nx, ny = b->ny;
    int first = nx, last = -1;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++)
            if (m01[(size_t)j * nx + i]) { if (i < first) first = i; if (i > last) last = i; }
    int c0 = 1, c1 = nx - 2;
#if WTP_MEX_WINDOW
    if (last < 0) c1 = 0;
    else { c0 = std::max(first - 1, 1); c1 = std::min(last + 1, nx - 2); }
#endif
    b->mex_win[2 * (size_t)member] = c0;
    b->mex_win[2 * (size_t)member + 1] = std::max(c1 - c0 + 1, 0);
}

// Zero the surface sums of members [first, first+count), in stream order.  Nothing to do while loads are off.
static int clear_surface_sums(wtp_batch *b, int first, int count)
{
    if (!b->loads) return WT_OK;
    const size_t off = (size_t)first * 2 * b->nx, n = (size_t)count * 2 * b->nx;
    HIP_TRY(hipMemsetAsync(b->s_rho + off, 0, n * sizeof(double), b->st));
    HIP_TRY(hipMemsetAsync(b->s_cnt + off, 0, n * sizeof(long long), b->st));
    return WT_OK;
}

// Zero the mean-field sums and the sample counts of members [first, first+count), in stream order.
static int zero_mean_sums(wtp_batch *b, int first, int count)
{
    HIP_TRY(hipMemsetAsync(b->m_sums + (size_t)first * b->m_stride, 0, (size_t)count * b->m_stride * sizeof(double), b->st));
    HIP_TRY(hipMemsetAsync(b->m_cnt + first, 0, (size_t)count * sizeof(long long), b->st));
    return WT_OK;
}

// The wall distances of members [first, first+count) back to 0.5 (half-way), in stream order.  Nothing to do while they are not held.
static int reset_wall_q(wtp_batch *b, int first, int count)
{
    if (!b->wq) return WT_OK;
    const long n = (long)count * b->q_stride;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 4096);
    with_dtype(b, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_fill_value<T>, dim3(blocks), dim3(256), 0, b->st, (T *)b->wq + (long)first * b->q_stride, n, T(0.5));
    });
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// The wall velocities of members [first, first+count) back to +0 (walls at rest), in stream order.  Nothing to do while they are not held.
static int reset_wall_u(wtp_batch *b, int first, int count)
{
    if (!b->wu) return WT_OK;
    HIP_TRY(hipMemsetAsync((char *)b->wu + (size_t)first * b->q_stride * b->esz, 0, (size_t)count * b->q_stride * b->esz, b->st));
    return WT_OK;
}

// Zero the probe sums and the sample counts of members [first, first+count), in stream order.  The points are kept.
static int zero_probe_sums(wtp_batch *b, int first, int count)
{
    const size_t P = (size_t)b->pb_n;
    HIP_TRY(hipMemsetAsync(b->pb_sums + (size_t)first * 3 * P, 0, (size_t)count * 3 * P * sizeof(double), b->st));
    HIP_TRY(hipMemsetAsync(b->pb_cnt + first, 0, (size_t)count * sizeof(long long), b->st));
    return WT_OK;
}

// What restarts the time statistics of members [first, first+count): the surface sums, the mean fields and the probe sums, each if enabled.
static int clear_sums(wtp_batch *b, int first, int count)
{
    WT_TRY(clear_surface_sums(b, first, count));
    if (b->mean) WT_TRY(zero_mean_sums(b, first, count));
    return b->probes ? zero_probe_sums(b, first, count) : WT_OK;
}

extern "C" int wtp_set_masks(wtp_batch *b, int first, int count, const uint8_t *masks)
{
    WT_TRY(check_batch(b));
    if (!masks) return fail(WT_ERR_ARG, "masks is null");
    WT_TRY(check_members(b, first, count));
    HIP_TRY(hipSetDevice(b->device));
    const Geom &g = b->g;
    const size_t n = (size_t)b->nx * b->ny;
    WT_TRY(ensure_stage(b, n));
    std::vector<uint8_t> m01(n);
    HIP_TRY(hipStreamSynchronize(b->st));        // the stage may still feed an earlier conversion; steps before this call see the old mask
    for (int k = 0; k < count; k++) {
        const uint8_t *src = masks + (size_t)k * n;
        for (size_t q = 0; q < n; q++) m01[q] = src[q] ? 1 : 0;
        surface_rows(b, first + k, m01.data());
        mex_window(b, first + k, m01.data());
        WT_TRY(clear_sums(b, first + k, 1));                    // the member's surface cells moved; a mean across two bodies means nothing
        WT_TRY(reset_wall_q(b, first + k, 1));                  // a wall distance belongs to a mask
        WT_TRY(reset_wall_u(b, first + k, 1));                  // ... and so does a wall velocity
        HIP_TRY(hipMemcpy(b->stage, m01.data(), n, hipMemcpyHostToDevice));
        uint8_t *mm = b->mask + (long)(first + k) * b->ms.mask;
        dim3 blk(32, 8), grd((b->nx + 31) / 32, (b->ny + 31) / 32);
        // [NY][NX] rows -> column i at row i + 1 of the padded mask (pad columns and rows past NY stay 0 from wtp_create)
        hipLaunchKernelGGL(k_rows_to_cols<uint8_t>, grd, blk, 0, b->st, (const uint8_t *)b->stage, mm + g.pitch, 0, b->nx, b->ny,
                           g.pitch, (long)b->nx);
        HIP_TRY(hipGetLastError());
        if (classify_tiles(mm, b->tiles + (long)(first + k) * b->ms.tiles, g, b->tiles_per_col, b->st) != 0)
            return fail(WT_ERR_HIP, "k_classify launch failed: %s", hipGetErrorString(hipGetLastError()));
        HIP_TRY(hipStreamSynchronize(b->st));
        b->mask_set[(size_t)(first + k)] = 1;
    }
    if (b->mex)                                  // (the stream is idle: samples already enqueued read the previous windows)
        HIP_TRY(hipMemcpy(b->x_win + 2 * (size_t)first, b->mex_win.data() + 2 * (size_t)first, (size_t)count * 2 * sizeof(int32_t),
                          hipMemcpyHostToDevice));
    return WT_OK;
}

// The equilibrium populations of a uniform flow (u0, v0) at rho = 1, evaluated in double as equilibrium_init evaluates them and rounded
// to T once: w (1 + 3 eu + 4.5 eu eu - 1.5 uu) with eu = ex u0 + ey v0 and uu = u0 u0 + v0 v0.  With v0 = 0 these are equilibrium_init's bits.
template <typename T>
static Init9<T> wind_init(double u0, double v0)
{
    const double w0 = 4.0 / 9.0, ws = 1.0 / 9.0, wd = 1.0 / 36.0;
    Init9<T> iv;
    for (int k = 0; k < 9; k++) {
        const double w = (k == 0) ? w0 : (k <= 4 ? ws : wd);
        const double eu = ex_of(k) * u0 + ey_of(k) * v0, uu = u0 * u0 + v0 * v0;
        iv.v[k] = (T)(w * (1 + 3 * eu + 4.5 * eu * eu - 1.5 * uu));
    }
    iv.u0 = (T)u0;
    return iv;
}

// The fp start values of member m, and its cross-flow v0: wind_init with an inclined free stream, else wt_init_equilibrium's values and 0.
template <typename T>
static Init9<T> start_values(const wtp_batch *b, int m, double u0, double *v0)
{
    *v0 = b->wind ? b->wind_host[(size_t)m] : 0.0;
    return b->wind ? wind_init<T>(u0, *v0) : equilibrium_init<T>(u0);
}

template <typename T>
static int init_impl(wtp_batch *b, const double *u0)
{
    for (int m = 0; m < b->members; m++) {
        double v0;
        const Init9<T> iv = start_values<T>(b, m, u0[m], &v0);
        if (b->wind)
            hipLaunchKernelGGL(k_fill_wind<T>, dim3(2048), dim3(256), 0, b->st, fptr<T>(b, 0, m), fptr<T>(b, 1, m), macro_of<T>(b, m), b->g, iv, (T)v0);
        else
            hipLaunchKernelGGL(k_fill_equilibrium<T>, dim3(2048), dim3(256), 0, b->st, fptr<T>(b, 0, m), fptr<T>(b, 1, m), macro_of<T>(b, m), b->g, iv);
        HIP_TRY(hipGetLastError());
    }
    return WT_OK;
}

// The start state of a half batch: the fp32 start values of init_impl<float>, stored through Store by k_fill_half.
static int init_half(wtp_batch *b, const double *u0)
{
    for (int m = 0; m < b->members; m++) {
        double v0;
        const Init9<float> iv = start_values<float>(b, m, u0[m], &v0);
        hipLaunchKernelGGL(k_fill_half, dim3(2048), dim3(256), 0, b->st, fptr<half_t>(b, 0, m), fptr<half_t>(b, 1, m), macro_of<float>(b, m),
                           b->g, iv, (float)v0);
        HIP_TRY(hipGetLastError());
    }
    return WT_OK;
}

extern "C" int wtp_init_equilibrium(wtp_batch *b, const double *u0)
{
    WT_TRY(check_batch(b));
    if (!u0) return fail(WT_ERR_ARG, "u0 is null");
    for (int m = 0; m < b->members; m++)
        if (!std::isfinite(u0[m])) return fail(WT_ERR_ARG, "u0[%d] must be finite", m);
    HIP_TRY(hipSetDevice(b->device));
    if (b->storage == WTP_STORE_HALF) WT_TRY(init_half(b, u0));
    else WT_TRY(with_dtype(b, [&](auto t) { return init_impl<decltype(t)>(b, u0); }));
    b->cur = 0;
    b->inited = true;
    b->macro_stale = false;
    b->steps_done = 0;
    b->h_step.clear();
    b->v_since = 0;                              // (the far-field vortex keeps its strengths)
    b->v_step.clear();
    return clear_sums(b, 0, b->members);
}

// ------------------------------------------------------------------------------------------
// stepping
// ------------------------------------------------------------------------------------------
static int check_ready(const wtp_batch *b)
{
    if (!b->inited) return fail(WT_ERR_STATE, "wtp_init_equilibrium has not been called");
    for (int m = 0; m < b->members; m++)
        if (!b->mask_set[(size_t)m]) return fail(WT_ERR_STATE, "member %d has no mask (wtp_set_masks)", m);
    return WT_OK;
}

// The macroscopic planes belong to the populations: not after a write, until a step has emitted.
static int check_macro(const wtp_batch *b)
{
    if (b->macro_stale)
        return fail(WT_ERR_STATE, "the macroscopic planes are those of the state before wtp_write_f / wtp_write_stored: run wtp_step (nsteps >= 1) first");
    return WT_OK;
}

// tau and U0 of every member, rounded to T exactly as wt_step rounds them; uploaded only when they change
template <typename T>
static int upload_params(wtp_batch *b, const double *tau, const double *u0)
{
    std::vector<double> want((size_t)b->members * 2);
    for (int m = 0; m < b->members; m++) { want[2 * (size_t)m] = tau[m]; want[2 * (size_t)m + 1] = u0[m]; }
    if (want == b->params_host) return WT_OK;
    std::vector<T> v(want.size());
    for (size_t q = 0; q < want.size(); q++) v[q] = (T)want[q];
    HIP_TRY(hipStreamSynchronize(b->st));        // steps already enqueued read the previous values
    HIP_TRY(hipMemcpy(b->params, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    b->params_host.swap(want);
    return WT_OK;
}

// wt_forces of every member on the last emitted state, into four [B] arrays of the device.
template <typename T>
static int launch_forces_to(wtp_batch *b, double *fx, double *fy, long long *surf, long long *rev)
{
    hipLaunchKernelGGL(k_forces_batch<T>, dim3((unsigned)b->nb, (unsigned)b->members), dim3(256), 0, b->st,
                       (const T *)b->macro, (const uint8_t *)b->mask, b->g, b->ms, b->nb, b->partials, b->tickets, fx, fy, surf, rev);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

template <typename T>
static int launch_forces(wtp_batch *b, int row)
{
    const SampleTable &t = b->forces;
    return launch_forces_to<T>(b, t.at<double>(0, row), t.at<double>(1, row), t.at<long long>(2, row), t.at<long long>(3, row));
}

// The far-field vortex's kernel over every table entry of every member.  UPDATE: the strengths of v_str[v_par] move by the forces in
// v_forces into the other half, with log row `row`, and the tables follow the new ones (the caller flips v_par); else the tables are
// built from v_str[v_par] as it is.
template <typename T, bool UPDATE>
static int launch_far_vortex(wtp_batch *b, int row)
{
    const size_t B = (size_t)b->members;
    const int entries = b->ny + 2 * b->nx;
    const double *forces = (const double *)b->v_forces;
    hipLaunchKernelGGL((k_far_vortex<T, UPDATE>), dim3((unsigned)((entries + kVortexBlock - 1) / kVortexBlock), (unsigned)B), dim3(kVortexBlock), 0, b->st,
                       (T *)b->prof, b->p_stride, b->g.pitch, b->p_nxp, b->nx, b->ny, b->v_set, (const double *)b->v_member, forces, forces + B,
                       (const double *)(b->v_str + (size_t)b->v_par * 2 * B), b->v_str + (size_t)(1 - b->v_par) * 2 * B,
                       UPDATE ? b->v_log + (size_t)row * B : nullptr, (long)b->v_cap * (long)B, UPDATE ? b->v_clip + (size_t)row * B : nullptr);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// One update of the far-field vortex from the last emitted state, logged as row v_step.size() with the current step count: the force
// read-out into the update's own scratch row, then the update and the tables.  The caller has checked that the log has room.
template <typename T>
static int far_vortex_update_now(wtp_batch *b)
{
    const size_t B = (size_t)b->members;
    double *f = (double *)b->v_forces;
    long long *n = (long long *)b->v_forces;
    WT_TRY(launch_forces_to<T>(b, f, f + B, n + 2 * B, n + 3 * B));
    WT_TRY((launch_far_vortex<T, true>(b, (int)b->v_step.size())));
    b->v_par = 1 - b->v_par;
    b->v_step.push_back(b->steps_done);
    return WT_OK;
}

// The surface loads of the last emitted state: Mz into row `row` of the history; accumulate: also add to the surface sums.
template <typename T>
static int launch_loads(wtp_batch *b, int row, bool accumulate)
{
    hipLaunchKernelGGL(k_loads_batch<T>, dim3((unsigned)((b->nx + kLoadsWaves - 1) / kLoadsWaves), (unsigned)b->members),
                       dim3(kLoadsWaves * 64), 0, b->st, (const T *)b->macro, (const uint8_t *)b->mask, b->g, b->ms, (const double *)b->l_ref, b->l_col, b->l_tickets,
                       b->moment.at<double>(0, row), b->s_rho, b->s_cnt, accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// The momentum exchange of the current lattice into row `row` of its history.
template <typename T>
static int launch_mex(wtp_batch *b, int row)
{
    int widest = 1;                              // (a batch without a body still runs one block per member, which writes zeros)
    for (int m = 0; m < b->members; m++) widest = std::max(widest, (int)b->mex_win[2 * (size_t)m + 1]);
    const SampleTable &t = b->xforces;
    const dim3 grid((unsigned)((widest + kLoadsWaves - 1) / kLoadsWaves), (unsigned)b->members), block(kLoadsWaves * 64);
    const auto launch = [&](auto e, auto link) {             // e: the lattice's stored element
        using E = decltype(e);
        hipLaunchKernelGGL((k_mex_batch<E, decltype(link)>), grid, block, 0, b->st, (const E *)fptr<E>(b, b->cur, 0), (const uint8_t *)b->mask, b->g,
                           b->ms, (const double *)b->x_ref, (const int32_t *)b->x_win, b->x_col, b->x_tickets, t.at<double>(0, row),
                           t.at<double>(1, row), t.at<double>(2, row), t.at<long long>(3, row), link);
    };
    const T *wq = (const T *)b->wq, *wu = (const T *)b->wu;
    if (b->storage == WTP_STORE_HALF) launch(half_t(), LinkHalfway<float>{});
    else if (b->wallvel) launch(T(), LinkMoving<T>{wq, b->q_stride, wu, b->q_stride});
    else if (b->ibb) launch(T(), LinkInterp<T>{wq, b->q_stride});
    else launch(T(), LinkHalfway<T>{});
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// The emitted fields of every member added to its mean-field sums, and one sample to its count.
template <typename T>
static int launch_mean(wtp_batch *b)
{
    const long lanes = (long)b->nx * (b->m_pitch / WTP_MEAN_ROWS);
    hipLaunchKernelGGL(k_mean_batch<T>, dim3((unsigned)((lanes + 255) / 256), (unsigned)b->members), dim3(256), 0, b->st,
                       (const T *)b->macro, b->g, b->ms, b->m_sums, b->m_stride, b->m_pitch, b->m_cnt);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// The emitted fields of every member sampled at its probe points and added to the points' sums, and one sample to its count.
template <typename T>
static int launch_probes(wtp_batch *b)
{
    hipLaunchKernelGGL((k_probe_batch<T, true>), dim3((unsigned)((b->pb_n + 255) / 256), (unsigned)b->members), dim3(256), 0, b->st,
                       (const T *)b->macro, b->g, b->ms, b->pb_n, (const long long *)b->pb_off, (const double *)b->pb_w, b->pb_sums, b->pb_cnt);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

// One sample of the state the last step left: every read-out that is enabled, into row `row` of its table.
template <typename T>
static int sample_into(wtp_batch *b, int row)
{
    WT_TRY(launch_forces<T>(b, row));
    if (b->loads) WT_TRY(launch_loads<T>(b, row, true));
    if (b->mex) WT_TRY(launch_mex<T>(b, row));
    if (b->mean) WT_TRY(launch_mean<T>(b));
    if (b->probes) WT_TRY(launch_probes<T>(b));
    return WT_OK;
}

// f(std::integral_constant<int, v>()) for the v in [0, N) that `v` holds: a run-time switch handed on as a compile-time value.
template <int N, typename F>
static void with_constant(int v, F f)
{
    if constexpr (N > 0) {
        if (v == N - 1) f(std::integral_constant<int, N - 1>());
        else with_constant<N - 1>(v, f);
    }
}

// The step variant that the batch's switches select: launch(EMIT, COLL, WALL, FAR) with the variant's template arguments as compile-time
// values.  The two-relaxation-time collisions take the inclined far field where the free stream is axial (k_step_batch).
template <typename Launch>
static void with_step_variant(const wtp_batch *b, bool emit, Launch launch)
{
    const int coll = b->trt ? (b->les ? COLLIDE_TRT_LES : COLLIDE_TRT) : (b->les ? COLLIDE_LES : COLLIDE_BGK);
    const int wall = b->wallvel ? WALL_MOVING : (b->ibb ? WALL_INTERP : WALL_HALFWAY);
    const int far = b->profile ? FAR_PROFILE : (b->wind || b->trt ? FAR_INCLINED : FAR_AXIAL);
    with_constant<2>(emit, [&](auto EMIT) { with_constant<4>(coll, [&](auto COLL) { with_constant<3>(wall, [&](auto WALL) {
        with_constant<3>(far, [&](auto FAR) {
            if constexpr (!coll_is_trt(COLL) || FAR != FAR_AXIAL) launch(EMIT, COLL, WALL, FAR);
        }); }); }); });
}

// The model arguments of one variant from the batch, with values of type T.  A two-relaxation-time variant of a batch without
// wtp_enable_wind reads the array of zeros as its cross-flow.
template <typename T, int COLL, int WALL, int FAR>
static StepModel<T, COLL, WALL, FAR> step_model(const wtp_batch *b, int rev)
{
    StepModel<T, COLL, WALL, FAR> a;
    if constexpr (coll_has_les(COLL)) a.cles = (const T *)b->les_c;
    if constexpr (wall_has_links(WALL)) { a.wq = (const T *)b->wq; a.qstride = b->q_stride; }
    if constexpr (WALL == WALL_MOVING) { a.wu = (const T *)b->wu; a.ustride = b->q_stride; }
    if constexpr (FAR == FAR_INCLINED) a.vwind = (const T *)(b->wind ? b->wind_v : b->zero_v);
    if constexpr (coll_is_trt(COLL)) a.lam = (const T *)b->trt_lam;
    if constexpr (FAR == FAR_PROFILE) { a.prof = (const T *)b->prof; a.pstride = b->p_stride; a.nxp = b->p_nxp; }
    a.rev = rev;
    return a;
}

// The stepping loop of wtp_step: which steps sample and which emit, the flip of the lattices, the step count and the history rows.
// `launch(emit, rev)` enqueues one step of every member from the current lattice into the other; T is the type of the read-outs.
// While the device-side far-field vortex is on, the step that brings `since` to a multiple of `every` at an absolute count of at least
// `after` also emits and is followed, behind its sample, by the update of the strengths and the tables (far_vortex_update_now).
template <typename T, typename Launch>
static int step_loop(wtp_batch *b, int nsteps, int sample_every, Launch launch)
{
    for (int s = 0; s < nsteps; s++) {
        const long long n = b->steps_done + 1;
        const bool sample = sample_every > 0 && n % sample_every == 0;
        const bool update = b->vortex && (b->v_since + 1) % b->v_every == 0 && n >= b->v_after;
        const bool emit = sample || update || s + 1 == nsteps;
        launch(emit, (int)(b->steps_done & 1));
        HIP_TRY(hipGetLastError());
        b->cur = 1 - b->cur;
        b->steps_done = n;
        if (b->vortex) b->v_since += 1;
        if (sample) {
            WT_TRY(sample_into<T>(b, (int)b->h_step.size()));
            b->h_step.push_back(n);
        }
        if (update) WT_TRY(far_vortex_update_now<T>(b));
    }
    return WT_OK;
}

// The updates of the far-field vortex that the next nsteps steps hold: the s in [1, nsteps] with (since + s) % every == 0 and
// steps_done + s >= after.
static long long far_vortex_updates(const wtp_batch *b, int nsteps)
{
    if (!b->vortex) return 0;
    const long long s0 = std::max<long long>(1, b->v_after - b->steps_done);
    if (s0 > nsteps) return 0;
    return (b->v_since + nsteps) / b->v_every - (b->v_since + s0 - 1) / b->v_every;
}

// The steps of a half batch: k_step_half_batch, with the fp32 read-outs.  wtp_enable_ibb and wtp_enable_far_profile refuse a half
// batch, so the variants that k_step_half_batch does not have are never selected; were one selected, that is an error and no launch.
static int step_half(wtp_batch *b, int nsteps, int sample_every)
{
    if (b->ibb || b->profile) return fail(WT_ERR_STATE, "a half batch has no step kernel with interpolated walls or a far-field profile");
    const dim3 grid(half_step_blocks(b->g), (unsigned)b->members), block(256);
    return step_loop<float>(b, nsteps, sample_every, [&](bool emit, int rev) {
        with_step_variant(b, emit, [&](auto EMIT, auto COLL, auto WALL, auto FAR) {
            if constexpr (WALL == WALL_HALFWAY && FAR != FAR_PROFILE)
                hipLaunchKernelGGL((k_step_half_batch<EMIT != 0, COLL, FAR>), grid, block, 0, b->st, (const half_t *)fptr<half_t>(b, b->cur, 0),
                                   fptr<half_t>(b, 1 - b->cur, 0), macro_of<float>(b, 0), (const uint8_t *)b->mask, b->g, b->ms,
                                   (const float *)b->params, step_model<float, COLL, WALL, FAR>(b, rev));
        });
    });
}

// The steps of a native batch: the tiled kernel that the collision, the wall rule and the far field select.
template <typename T>
static int step_impl(wtp_batch *b, int nsteps, int sample_every)
{
    const long ntiles = (long)b->g.nxl * b->tiles_per_col;
    const dim3 grid((unsigned)((ntiles + 3) / 4), (unsigned)b->members), block(256);
    return step_loop<T>(b, nsteps, sample_every, [&](bool emit, int rev) {
        with_step_variant(b, emit, [&](auto EMIT, auto COLL, auto WALL, auto FAR) {
            hipLaunchKernelGGL((k_step_batch<T, EMIT != 0, WT_LOADMODE, COLL, WALL, FAR>), grid, block, 0, b->st, (const T *)fptr<T>(b, b->cur, 0),
                               fptr<T>(b, 1 - b->cur, 0), macro_of<T>(b, 0), (const uint8_t *)b->mask, (const uint8_t *)b->tiles, b->tiles_per_col,
                               b->g, b->ms, (const T *)b->params, step_model<T, COLL, WALL, FAR>(b, rev));
        });
    });
}

extern "C" int wtp_step(wtp_batch *b, int nsteps, const double *tau, const double *u0, int sample_every)
{
    WT_TRY(check_batch(b));
    if (nsteps < 0) return fail(WT_ERR_ARG, "nsteps < 0");
    if (sample_every < 0) return fail(WT_ERR_ARG, "sample_every < 0");
    if (!tau || !u0) return fail(WT_ERR_ARG, "tau or u0 is null");
    for (int m = 0; m < b->members; m++) {
        if (!(tau[m] > 0.0) || !std::isfinite(tau[m])) return fail(WT_ERR_ARG, "tau[%d] must be positive and finite", m);
        if (!std::isfinite(u0[m])) return fail(WT_ERR_ARG, "u0[%d] must be finite", m);
    }
    if (b->trt)                                  // tm = 0.5 + lam / (tp - 0.5) needs tp > 0.5 in the batch's dtype
        for (int m = 0; m < b->members; m++)
            if (!with_dtype(b, [&](auto t) { return (decltype(t))tau[m] > decltype(t)(0.5); }))
                return fail(WT_ERR_ARG, "tau[%d] must be above 0.5 in the batch's dtype while the two-relaxation-time collision is on", m);
    WT_TRY(check_ready(b));
    if (b->profile)
        for (int m = 0; m < b->members; m++)
            if (!b->prof_set[(size_t)m]) return fail(WT_ERR_STATE, "member %d has no far-field profile (wtp_set_far_profile)", m);
    if (sample_every > 0) {
        const long long samples = (b->steps_done + nsteps) / sample_every - b->steps_done / sample_every;
        if ((long long)b->h_step.size() + samples > b->cap)
            return fail(WT_ERR_STATE, "%lld samples would overflow the history (%zu of %d rows held): read it and wtp_clear_history",
                        samples, b->h_step.size(), b->cap);
    }
    if (const long long updates = far_vortex_updates(b, nsteps); (long long)b->v_step.size() + updates > b->v_cap)
        return fail(WT_ERR_STATE, "%lld updates would overflow the far-field vortex's log (%zu of %d rows held): read it and wtp_clear_history",
                    updates, b->v_step.size(), b->v_cap);
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(with_dtype(b, [&](auto t) {
        WT_TRY(upload_params<decltype(t)>(b, tau, u0));
        return b->storage == WTP_STORE_HALF ? step_half(b, nsteps, sample_every) : step_impl<decltype(t)>(b, nsteps, sample_every);
    }));
    if (nsteps > 0) b->macro_stale = false;      // the call's last step emitted
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// Smagorinsky subgrid viscosity
// ------------------------------------------------------------------------------------------
// One value per member, value_of(m) rounded to T once, into *dev (allocated on the first call) once the steps already enqueued, which
// read the previous values, have run.
template <typename T, typename Value>
static int upload_per_member(wtp_batch *b, void **dev, Value value_of)
{
    std::vector<T> v((size_t)b->members);
    for (size_t m = 0; m < v.size(); m++) v[m] = (T)value_of(m);
    WT_TRY(alloc_all({{dev, v.size() * sizeof(T)}}, "per-member values"));
    HIP_TRY(hipStreamSynchronize(b->st));
    HIP_TRY(hipMemcpy(*dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return WT_OK;
}

extern "C" int wtp_enable_les(wtp_batch *b, const double *cs)
{
    WT_TRY(check_batch(b));
    if (!cs) { b->les = false; return WT_OK; }   // (steps already enqueued were launched with the model on: stream order)
    for (int m = 0; m < b->members; m++)
        if (!std::isfinite(cs[m]) || cs[m] < 0.0 || cs[m] > 0.5) return fail(WT_ERR_ARG, "cs[%d] must be finite and in [0, 0.5]", m);
    HIP_TRY(hipSetDevice(b->device));
    const auto c = [&](size_t m) { return 18.0 * std::sqrt(2.0) * cs[m] * cs[m]; };      // c = 18 sqrt(2) Cs^2: formed left to right in double
    WT_TRY(with_dtype(b, [&](auto t) { return upload_per_member<decltype(t)>(b, &b->les_c, c); }));
    b->les = true;
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// two-relaxation-time collision
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_trt(wtp_batch *b, const double *magic)
{
    WT_TRY(check_batch(b));
    if (!magic) { b->trt = false; return WT_OK; }        // (steps already enqueued were launched with the model on: stream order)
    for (int m = 0; m < b->members; m++)
        if (!std::isfinite(magic[m]) || !(magic[m] > 0.0) || magic[m] > 1.0) return fail(WT_ERR_ARG, "magic[%d] must be finite and in (0, 1]", m);
    HIP_TRY(hipSetDevice(b->device));
    if (!b->zero_v) {
        WT_TRY(alloc_all({{&b->zero_v, (size_t)b->members * b->esz}}, "per-member values"));
        HIP_TRY(hipMemsetAsync(b->zero_v, 0, (size_t)b->members * b->esz, b->st));      // (+0 in either dtype)
    }
    const auto lam = [&](size_t m) { return magic[m]; };
    WT_TRY(with_dtype(b, [&](auto t) { return upload_per_member<decltype(t)>(b, &b->trt_lam, lam); }));
    b->trt = true;
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// inclined free stream
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_wind(wtp_batch *b, const double *v0)
{
    WT_TRY(check_batch(b));
    if (!v0) { b->wind = false; return WT_OK; }  // (steps already enqueued were launched with the model on: stream order)
    for (int m = 0; m < b->members; m++)
        if (!std::isfinite(v0[m]) || std::fabs(v0[m]) > 0.35) return fail(WT_ERR_ARG, "v0[%d] must be finite and in [-0.35, 0.35]", m);
    HIP_TRY(hipSetDevice(b->device));
    const auto v = [&](size_t m) { return v0[m]; };
    WT_TRY(with_dtype(b, [&](auto t) { return upload_per_member<decltype(t)>(b, &b->wind_v, v); }));
    b->wind_host.assign(v0, v0 + b->members);
    b->wind = true;
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// prescribed far-field profile
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_far_profile(wtp_batch *b, int on)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "a prescribed far-field profile"));
    if (!on) { b->profile = false; b->vortex = false; return WT_OK; }       // (steps already enqueued were launched with the model on: stream order)
    HIP_TRY(hipSetDevice(b->device));
    if (!b->prof) {
        const int nxp = (b->nx + 63) / 64 * 64;
        const long stride = member_stride((size_t)far_profile_elems(b->g.pitch, nxp) * b->esz, b->esz);
        const size_t bytes = (size_t)b->members * stride * b->esz;
        WT_TRY(alloc_all({{&b->prof, bytes}}, "far-field tables"));       // (on a failure the batch goes on with its uniform far field)
        b->p_stride = stride; b->p_nxp = nxp;
        b->prof_set.assign((size_t)b->members, 0);
        HIP_TRY(hipMemsetAsync(b->prof, 0, bytes, b->st));      // (the entries no cell reads, rows past NY and columns past NX, hold +0)
    }
    b->profile = true;
    return WT_OK;
}

// One entry of a table: finite, rho in [0.5, 2], ux^2 + uy^2 <= 0.35^2 (the bounds of the stability net).  False for a NaN.
static bool far_entry_ok(double rho, double ux, double uy)
{
    return rho >= 0.5 && rho <= 2.0 && std::isfinite(ux) && std::isfinite(uy) && ux * ux + uy * uy <= 0.35 * 0.35;
}

template <typename T>
static int set_far_profile_impl(wtp_batch *b, int first, int count, const T *left, const T *bottom, const T *top)
{
    const size_t nx = (size_t)b->nx, ny = (size_t)b->ny;
    const struct { const T *v; size_t n; const char *name; } tabs[3] = {{left, ny, "left"}, {bottom, nx, "bottom"}, {top, nx, "top"}};
    for (const auto &t : tabs)
        for (size_t k = 0; k < (size_t)count; k++)
            for (size_t e = 0; e < t.n; e++) {
                const T *p = t.v + k * 3 * t.n + e;
                if (!far_entry_ok((double)p[0], (double)p[t.n], (double)p[2 * t.n]))
                    return fail(WT_ERR_ARG, "entry %zu of `%s` of member %d is not finite with rho in [0.5, 2] and a speed of at most 0.35", e, t.name,
                                first + (int)k);
            }
    HIP_TRY(hipSetDevice(b->device));
    const size_t pitch = (size_t)b->g.pitch, nxp = (size_t)b->p_nxp, elems = (size_t)far_profile_elems(b->g.pitch, b->p_nxp);
    std::vector<T> host(elems * (size_t)count, T(0.0));          // the device layout of FarProfile, members packed
    for (size_t k = 0; k < (size_t)count; k++) {
        T *d = host.data() + k * elems;
        for (size_t p = 0; p < 3; p++) {
            std::memcpy(d + p * pitch, left + (k * 3 + p) * ny, ny * sizeof(T));
            std::memcpy(d + 3 * pitch + p * nxp, bottom + (k * 3 + p) * nx, nx * sizeof(T));
            std::memcpy(d + 3 * pitch + (3 + p) * nxp, top + (k * 3 + p) * nx, nx * sizeof(T));
        }
    }
    HIP_TRY(hipStreamSynchronize(b->st));        // steps already enqueued read the previous values
    for (size_t k = 0; k < (size_t)count; k++) {
        HIP_TRY(hipMemcpy(reinterpret_cast<T *>(b->prof) + (long)(first + (int)k) * b->p_stride, host.data() + k * elems, elems * sizeof(T),
                          hipMemcpyHostToDevice));
        b->prof_set[(size_t)first + k] = 1;
    }
    return WT_OK;
}

extern "C" int wtp_set_far_profile(wtp_batch *b, int first, int count, const void *left, const void *bottom, const void *top)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "a prescribed far-field profile"));
    if (!left || !bottom || !top) return fail(WT_ERR_ARG, "left, bottom or top is null");
    WT_TRY(check_members(b, first, count));
    if (!b->prof) return fail(WT_ERR_STATE, "the far-field profile has never been enabled (wtp_enable_far_profile)");
    if (b->vortex) return fail(WT_ERR_STATE, "the device-side far-field vortex owns the tables (wtp_enable_far_vortex with every = 0 hands them back)");
    return with_dtype(b, [&](auto t) {
        using T = decltype(t);
        return set_far_profile_impl(b, first, count, (const T *)left, (const T *)bottom, (const T *)top);
    });
}

// The device layout of FarProfile of members [first, first + count) unpacked into wtp_set_far_profile's host layouts.
template <typename T>
static int read_far_profile_impl(wtp_batch *b, int first, int count, T *left, T *bottom, T *top)
{
    const size_t nx = (size_t)b->nx, ny = (size_t)b->ny;
    const size_t pitch = (size_t)b->g.pitch, nxp = (size_t)b->p_nxp, elems = (size_t)far_profile_elems(b->g.pitch, b->p_nxp);
    std::vector<T> host(elems);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    for (size_t k = 0; k < (size_t)count; k++) {
        HIP_TRY(hipMemcpy(host.data(), reinterpret_cast<const T *>(b->prof) + (long)(first + (int)k) * b->p_stride, elems * sizeof(T), hipMemcpyDeviceToHost));
        const T *d = host.data();
        for (size_t p = 0; p < 3; p++) {
            if (left) std::memcpy(left + (k * 3 + p) * ny, d + p * pitch, ny * sizeof(T));
            if (bottom) std::memcpy(bottom + (k * 3 + p) * nx, d + 3 * pitch + p * nxp, nx * sizeof(T));
            if (top) std::memcpy(top + (k * 3 + p) * nx, d + 3 * pitch + (3 + p) * nxp, nx * sizeof(T));
        }
    }
    return WT_OK;
}

extern "C" int wtp_read_far_profile(wtp_batch *b, int first, int count, void *left, void *bottom, void *top)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_members(b, first, count));
    if (!b->prof) return fail(WT_ERR_STATE, "the far-field profile has never been enabled (wtp_enable_far_profile)");
    for (int m = first; m < first + count; m++)
        if (!b->prof_set[(size_t)m]) return fail(WT_ERR_STATE, "member %d has no far-field profile (wtp_set_far_profile)", m);
    return with_dtype(b, [&](auto t) {
        using T = decltype(t);
        return read_far_profile_impl(b, first, count, (T *)left, (T *)bottom, (T *)top);
    });
}

// ------------------------------------------------------------------------------------------
// device-side far-field vortex (include/wt_polar.h "Device-side far-field vortex")
// ------------------------------------------------------------------------------------------
// A pair of strengths is inside the clip: finite, with sqrt(s*s + q*q)/bound <= 0.1.  False for a NaN.
static bool far_vortex_pair_ok(double s, double q, double bound)
{
    return std::isfinite(s) && std::isfinite(q) && std::sqrt(s * s + q * q) / bound <= 0.1;
}

// All tables from the current strengths, behind whatever is enqueued.
static int far_vortex_tables(wtp_batch *b)
{
    return with_dtype(b, [&](auto t) { return launch_far_vortex<decltype(t), false>(b, 0); });
}

extern "C" int wtp_enable_far_vortex(wtp_batch *b, int every, int64_t after, double relax, double u_ref, int with_source, double xc, double yc,
                                     const double *u_far, const double *v_far, const double *cos_a, const double *sin_a, int log_cap)
{
    WT_TRY(check_batch(b));
    if (every == 0) { b->vortex = false; return WT_OK; }      // (updates already enqueued were launched with the model on: stream order)
    WT_TRY(check_native(b, "a prescribed far-field profile"));
    if (!b->profile) return fail(WT_ERR_STATE, "the far-field profile is not enabled (wtp_enable_far_profile)");
    if (every < 0) return fail(WT_ERR_ARG, "every must be >= 0 (got %d)", every);
    if (after < 0) return fail(WT_ERR_ARG, "after must be >= 0 (got %lld)", (long long)after);
    if (!(relax > 0.0 && relax <= 1.0)) return fail(WT_ERR_ARG, "relax must be in (0, 1]");
    if (!(u_ref > 0.0) || !std::isfinite(u_ref)) return fail(WT_ERR_ARG, "u_ref must be positive and finite");
    if (with_source != 0 && with_source != 1) return fail(WT_ERR_ARG, "with_source must be 0 or 1 (got %d)", with_source);
    if (!std::isfinite(xc) || !std::isfinite(yc)) return fail(WT_ERR_ARG, "xc and yc must be finite");
    const double bound = std::min(std::min(xc - 0.5, yc - 0.5), ((double)b->ny - 0.5) - yc);
    if (!(bound >= 1.0)) return fail(WT_ERR_ARG, "(xc, yc) must lie at least one cell from the nearest far-field cell centre (bound %g)", bound);
    if (log_cap < 0) return fail(WT_ERR_ARG, "log_cap must be >= 0 (got %d)", log_cap);
    if (!u_far || !v_far || !cos_a || !sin_a) return fail(WT_ERR_ARG, "u_far, v_far, cos_a or sin_a is null");
    const size_t B = (size_t)b->members;
    for (size_t m = 0; m < B; m++) {
        if (!(u_far[m] * u_far[m] + v_far[m] * v_far[m] <= 0.25 * 0.25))       // (false for a NaN)
            return fail(WT_ERR_ARG, "the far stream of member %d must be finite with a speed of at most 0.25", (int)m);
        if (!(std::fabs(cos_a[m]) <= 1.0) || !(std::fabs(sin_a[m]) <= 1.0))
            return fail(WT_ERR_ARG, "cos_a and sin_a of member %d must be finite and in [-1, 1]", (int)m);
    }
    HIP_TRY(hipSetDevice(b->device));
    std::vector<double> held(2 * B, 0.0);
    if (b->v_str) {                              // the strengths are kept: they have to fit the new bound
        HIP_TRY(hipStreamSynchronize(b->st));
        HIP_TRY(hipMemcpy(held.data(), b->v_str + (size_t)b->v_par * 2 * B, 2 * B * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t m = 0; m < B; m++)
            if (!far_vortex_pair_ok(held[m], held[B + m], bound))
                return fail(WT_ERR_ARG, "the strengths held by member %d induce more than 0.1 at the new bound %g", (int)m, bound);
    }
    // the buffers: everything of the first enable at once, a log of another size on a later one
    const bool relog = !b->v_log || log_cap != b->v_cap;
    void *member = b->v_member, *str = b->v_str, *forces = b->v_forces, *log = relog ? nullptr : b->v_log, *clip = relog ? nullptr : b->v_clip;
    const size_t rows = (size_t)std::max(log_cap, 1);
    HIP_TRY(hipStreamSynchronize(b->st));        // updates already enqueued read the previous settings and write the previous log
    WT_TRY(alloc_all({{&member, 4 * B * sizeof(double)}, {&str, 4 * B * sizeof(double)}, {&forces, 4 * B * 8},
                      {&log, 4 * rows * B * sizeof(double)}, {&clip, rows * B * sizeof(int32_t)}}, "far-field vortex's buffers"));
    if (hipError_t e = b->v_str ? hipSuccess : hipMemcpy(str, held.data(), 2 * B * sizeof(double), hipMemcpyHostToDevice)) {      // (zeros, into half 0)
        (void)hipGetLastError();                 // (the batch goes on as it was: later launches must not see this error)
        for (void *p : {b->v_member ? nullptr : member, str, b->v_forces ? nullptr : forces, relog ? log : nullptr, relog ? clip : nullptr}) if (p) (void)hipFree(p);
        return fail(e == hipErrorOutOfMemory ? WT_ERR_OOM : WT_ERR_HIP, "the far-field vortex's buffers could not be set up: %s", hipGetErrorString(e));
    }
    if (!b->v_str) b->v_par = 0;
    b->v_member = (double *)member; b->v_str = (double *)str; b->v_forces = forces;
    if (relog) {
        if (b->v_log) (void)hipFree(b->v_log);
        if (b->v_clip) (void)hipFree(b->v_clip);
        b->v_log = (double *)log; b->v_clip = (int32_t *)clip;
    }
    std::vector<double> set(4 * B);
    for (size_t m = 0; m < B; m++) { set[m] = u_far[m]; set[B + m] = v_far[m]; set[2 * B + m] = cos_a[m]; set[3 * B + m] = sin_a[m]; }
    HIP_TRY(hipMemcpy(b->v_member, set.data(), set.size() * sizeof(double), hipMemcpyHostToDevice));
    b->v_set.relax = relax; b->v_set.den = (2.0 * M_PI) * u_ref; b->v_set.bound = bound; b->v_set.xc = xc; b->v_set.yc = yc;
    b->v_set.with_source = with_source;
    b->v_every = every; b->v_after = after; b->v_since = 0; b->v_cap = log_cap;
    b->v_step.clear();
    b->vortex = true;
    b->prof_set.assign(B, 1);
    return far_vortex_tables(b);
}

static int check_far_vortex(const wtp_batch *b)
{
    if (!b->vortex) return fail(WT_ERR_STATE, "the device-side far-field vortex is not enabled (wtp_enable_far_vortex)");
    return WT_OK;
}

extern "C" int wtp_set_far_vortex(wtp_batch *b, const double *strength, const double *source)
{
    WT_TRY(check_batch(b));
    if (!strength || !source) return fail(WT_ERR_ARG, "strength or source is null");
    WT_TRY(check_far_vortex(b));
    const size_t B = (size_t)b->members;
    for (size_t m = 0; m < B; m++)
        if (!far_vortex_pair_ok(strength[m], source[m], b->v_set.bound))
            return fail(WT_ERR_ARG, "strength and source of member %d must be finite and induce at most 0.1 at the bound %g", (int)m, b->v_set.bound);
    HIP_TRY(hipSetDevice(b->device));
    std::vector<double> pair(2 * B);
    for (size_t m = 0; m < B; m++) { pair[m] = strength[m]; pair[B + m] = source[m]; }
    HIP_TRY(hipStreamSynchronize(b->st));        // updates already enqueued read and replace the previous values
    HIP_TRY(hipMemcpy(b->v_str + (size_t)b->v_par * 2 * B, pair.data(), 2 * B * sizeof(double), hipMemcpyHostToDevice));
    return far_vortex_tables(b);
}

extern "C" int wtp_far_vortex(wtp_batch *b, double *strength, double *source)
{
    WT_TRY(check_batch(b));
    if (!strength || !source) return fail(WT_ERR_ARG, "strength or source is null");
    if (!b->v_str) return fail(WT_ERR_STATE, "the device-side far-field vortex has never been enabled (wtp_enable_far_vortex)");
    const size_t B = (size_t)b->members;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    const double *cur = b->v_str + (size_t)b->v_par * 2 * B;
    HIP_TRY(hipMemcpy(strength, cur, B * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(source, cur + B, B * sizeof(double), hipMemcpyDeviceToHost));
    return WT_OK;
}

extern "C" int wtp_far_vortex_update(wtp_batch *b)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_far_vortex(b));
    WT_TRY(check_ready(b));
    WT_TRY(check_macro(b));
    if ((int)b->v_step.size() >= b->v_cap)
        return fail(WT_ERR_STATE, "the far-field vortex's log is full (%d rows): read it and wtp_clear_history", b->v_cap);
    HIP_TRY(hipSetDevice(b->device));
    return with_dtype(b, [&](auto t) { return far_vortex_update_now<decltype(t)>(b); });
}

extern "C" int wtp_far_vortex_log(wtp_batch *b, int first, int count, int64_t *step, double *fx, double *fy, double *strength, double *source,
                                  int32_t *clipped)
{
    WT_TRY(check_batch(b));
    const int held = (int)b->v_step.size();
    if (first < 0 || count < 0 || first + count > held) return fail(WT_ERR_ARG, "rows [%d, %d) outside the %d held", first, first + count, held);
    if (count > 0) {
        const size_t B = (size_t)b->members, n = (size_t)count * B;
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->st));
        double *const dst[4] = {fx, fy, strength, source};
        for (int c = 0; c < 4; c++)
            if (dst[c]) HIP_TRY(hipMemcpy(dst[c], b->v_log + ((size_t)c * b->v_cap + first) * B, n * sizeof(double), hipMemcpyDeviceToHost));
        if (clipped) HIP_TRY(hipMemcpy(clipped, b->v_clip + (size_t)first * B, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (step) for (int r = 0; r < count; r++) step[r] = b->v_step[(size_t)(first + r)];
    }
    return held;
}

// ------------------------------------------------------------------------------------------
// interpolated bounce-back
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_ibb(wtp_batch *b, int on)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "interpolated bounce-back"));
    if (!on) { b->ibb = false; b->wallvel = false; return WT_OK; }   // (steps already enqueued were launched with the model on: stream order)
    HIP_TRY(hipSetDevice(b->device));
    if (!b->wq) {
        const long stride = member_stride((size_t)8 * b->g.plane * b->esz, b->esz);
        WT_TRY(alloc_all({{&b->wq, (size_t)b->members * stride * b->esz}}, "wall distances"));      // (on a failure the batch goes on with half-way walls)
        b->q_stride = stride;
        WT_TRY(reset_wall_q(b, 0, b->members));
    }
    b->ibb = true;
    return WT_OK;
}

// Eight [NY][NX] planes per member of members [first, first + count), from the host into the padded link-plane layout of `dev` (wq or wu:
// planes laid out like population planes 1..8, members q_stride elements apart), through the stage.  Every value has to pass `ok` (false
// for a NaN); the refusal names the value by `noun` and the interval by `bound`.
template <typename T, typename Ok>
static int upload_link_planes(wtp_batch *b, void *dev, int first, int count, const T *v, Ok ok, const char *noun, const char *bound)
{
    const size_t n = (size_t)b->nx * b->ny;
    for (size_t e = 0; e < (size_t)count * 8 * n; e++)
        if (!ok(v[e])) return fail(WT_ERR_ARG, "%s %zu of member %d is not in %s", noun, e % (8 * n), first + (int)(e / (8 * n)), bound);
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(ensure_stage(b, 8 * n * sizeof(T)));
    const Geom &g = b->g;
    for (int k = 0; k < count; k++) {
        HIP_TRY(hipStreamSynchronize(b->st));        // the stage may still feed an earlier conversion; steps before this call see the old values
        HIP_TRY(hipMemcpy(b->stage, v + (size_t)k * 8 * n, 8 * n * sizeof(T), hipMemcpyHostToDevice));
        T *dst = reinterpret_cast<T *>(dev) + (long)(first + k) * b->q_stride;
        dim3 blk(32, 8), grd((b->nx + 31) / 32, (b->ny + 31) / 32);
        for (int p = 0; p < 8; p++) {
            // [NY][NX] rows -> column i at row i + 1 of the padded plane (pad columns and rows past NY keep their default; nothing reads them)
            hipLaunchKernelGGL(k_rows_to_cols<T>, grd, blk, 0, b->st, reinterpret_cast<const T *>(b->stage) + (size_t)p * n,
                               dst + p * g.plane + g.pitch, 0, b->nx, b->ny, g.pitch, (long)b->nx);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(b->st));
    return WT_OK;
}

extern "C" int wtp_set_wall_q(wtp_batch *b, int first, int count, const void *q)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "interpolated bounce-back"));
    if (!q) return fail(WT_ERR_ARG, "q is null");
    WT_TRY(check_members(b, first, count));
    if (!b->wq) return fail(WT_ERR_STATE, "interpolated bounce-back has never been enabled (wtp_enable_ibb)");
    return with_dtype(b, [&](auto t) {
        using T = decltype(t);
        return upload_link_planes(b, b->wq, first, count, (const T *)q, [](T x) { return x > T(0.0) && x <= T(1.0); }, "wall distance", "(0, 1]");
    });
}

// ------------------------------------------------------------------------------------------
// wall velocity
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_wall_velocity(wtp_batch *b, int on)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "a wall velocity"));
    if (!on) { b->wallvel = false; return WT_OK; }   // (steps already enqueued were launched with the model on: stream order)
    if (!b->ibb) return fail(WT_ERR_STATE, "interpolated bounce-back is not enabled (wtp_enable_ibb)");
    HIP_TRY(hipSetDevice(b->device));
    if (!b->wu) {
        // the wall distances' layout and stride (on a failure the batch goes on with walls at rest)
        WT_TRY(alloc_all({{&b->wu, (size_t)b->members * b->q_stride * b->esz}}, "wall velocities"));
        WT_TRY(reset_wall_u(b, 0, b->members));
    }
    b->wallvel = true;
    return WT_OK;
}

extern "C" int wtp_set_wall_velocity(wtp_batch *b, int first, int count, const void *un)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_native(b, "a wall velocity"));
    if (!un) return fail(WT_ERR_ARG, "un is null");
    WT_TRY(check_members(b, first, count));
    if (!b->wu) return fail(WT_ERR_STATE, "wall velocity has never been enabled (wtp_enable_wall_velocity)");
    return with_dtype(b, [&](auto t) {
        using T = decltype(t);
        return upload_link_planes(b, b->wu, first, count, (const T *)un, [](T x) { return x >= T(-0.5) && x <= T(0.5); }, "wall velocity", "[-0.5, 0.5]");
    });
}

// ------------------------------------------------------------------------------------------
// read-backs
// ------------------------------------------------------------------------------------------
static int check_rows(const wtp_batch *b, int first, int count)
{
    const int held = (int)b->h_step.size();
    if (first < 0 || count < 0 || first + count > held) return fail(WT_ERR_ARG, "rows [%d, %d) outside the %d held", first, first + count, held);
    return WT_OK;
}

// Rows [first, first + count) of a table, once everything enqueued has run, into the destinations that are not null (one per
// column).  Row b->cap with count 1 is what an on-demand call reads back after its launch into the scratch row.
static int read_rows(wtp_batch *b, const SampleTable &t, int first, int count, void *const (&dst)[4])
{
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    return t.read(first, count, dst);
}

extern "C" int wtp_history(wtp_batch *b, int first, int count, int64_t *step, double *fx, double *fy, int64_t *surf, int64_t *rev)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_rows(b, first, count));
    WT_TRY(read_rows(b, b->forces, first, count, {fx, fy, surf, rev}));
    if (step) for (int r = 0; r < count; r++) step[r] = b->h_step[(size_t)(first + r)];
    return (int)b->h_step.size();
}

extern "C" int wtp_clear_history(wtp_batch *b)
{
    WT_TRY(check_batch(b));
    b->h_step.clear();                           // (rows are only written by later, stream-ordered reductions)
    b->v_step.clear();                           // (so are the rows of the far-field vortex's log)
    if (!b->loads && !b->mean && !b->probes) return WT_OK;
    HIP_TRY(hipSetDevice(b->device));
    return clear_sums(b, 0, b->members);
}

extern "C" int wtp_forces(wtp_batch *b, double *fx, double *fy, int64_t *surf, int64_t *rev)
{
    WT_TRY(check_batch(b));
    if (!fx || !fy || !surf || !rev) return fail(WT_ERR_ARG, "null output");
    WT_TRY(check_ready(b));
    WT_TRY(check_macro(b));
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(with_dtype(b, [&](auto t) { return launch_forces<decltype(t)>(b, b->cap); }));     // the scratch row
    return read_rows(b, b->forces, b->cap, 1, {fx, fy, surf, rev});
}

// ------------------------------------------------------------------------------------------
// surface loads
// ------------------------------------------------------------------------------------------
// The reference points of a moment read-out, (xref[m], yref[m]) of every member: checked, packed [B][2] and uploaded to *dev
// (allocated on the first call) once the samples already enqueued, which read the previous points, have run.
static int set_ref_points(wtp_batch *b, const double *xref, const double *yref, double **dev)
{
    const size_t B = (size_t)b->members;
    for (size_t m = 0; m < B; m++)
        if (!std::isfinite(xref[m]) || !std::isfinite(yref[m])) return fail(WT_ERR_ARG, "reference point of member %d must be finite", (int)m);
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(alloc_all({{(void **)dev, B * 2 * sizeof(double)}}, "reference points"));
    std::vector<double> ref(B * 2);
    for (size_t m = 0; m < B; m++) { ref[2 * m] = xref[m]; ref[2 * m + 1] = yref[m]; }
    HIP_TRY(hipStreamSynchronize(b->st));
    HIP_TRY(hipMemcpy(*dev, ref.data(), ref.size() * sizeof(double), hipMemcpyHostToDevice));
    return WT_OK;
}

extern "C" int wtp_enable_loads(wtp_batch *b, const double *xref, const double *yref)
{
    WT_TRY(check_batch(b));
    if (!xref || !yref) return fail(WT_ERR_ARG, "xref or yref is null");
    WT_TRY(set_ref_points(b, xref, yref, &b->l_ref));
    const size_t B = (size_t)b->members, cols = B * b->nx;
    WT_TRY(alloc_all({{(void **)&b->l_col, cols * sizeof(double)}, {(void **)&b->l_tickets, B * kTicketStride * sizeof(unsigned int)},
                      {(void **)&b->s_rho, 2 * cols * sizeof(double)}, {(void **)&b->s_cnt, 2 * cols * sizeof(long long)}}, "surface-load buffers"));
    WT_TRY(b->moment.alloc(1, (size_t)b->cap, B, "moment history"));
    HIP_TRY(hipMemsetAsync(b->l_tickets, 0, B * kTicketStride * sizeof(unsigned int), b->st));
    WT_TRY(b->moment.fill(1u, b->st));           // rows sampled before this call hold no Mz about these points
    b->loads = true;
    return clear_surface_sums(b, 0, b->members);
}

static int check_loads(const wtp_batch *b)
{
    if (!b->loads) return fail(WT_ERR_STATE, "surface loads are not enabled (wtp_enable_loads)");
    return WT_OK;
}

extern "C" int wtp_history_moment(wtp_batch *b, int first, int count, double *mz)
{
    WT_TRY(check_batch(b));
    if (!mz) return fail(WT_ERR_ARG, "mz is null");
    WT_TRY(check_rows(b, first, count));
    WT_TRY(check_loads(b));
    return read_rows(b, b->moment, first, count, {mz});
}

extern "C" int wtp_moment(wtp_batch *b, double *mz)
{
    WT_TRY(check_batch(b));
    if (!mz) return fail(WT_ERR_ARG, "mz is null");
    WT_TRY(check_loads(b));
    WT_TRY(check_ready(b));
    WT_TRY(check_macro(b));
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(with_dtype(b, [&](auto t) { return launch_loads<decltype(t)>(b, b->cap, false); }));     // the scratch row
    return read_rows(b, b->moment, b->cap, 1, {mz});
}

extern "C" int wtp_surface(wtp_batch *b, int member, double *rho_upper, double *rho_lower, int64_t *n_upper, int64_t *n_lower,
                           int32_t *j_upper, int32_t *j_lower)
{
    WT_TRY(check_batch(b));
    if (!rho_upper || !rho_lower || !n_upper || !n_lower || !j_upper || !j_lower) return fail(WT_ERR_ARG, "null output");
    WT_TRY(check_member(b, member));
    WT_TRY(check_loads(b));
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    const size_t nx = (size_t)b->nx, off = (size_t)member * 2 * nx;
    HIP_TRY(hipMemcpy(rho_upper, b->s_rho + off, nx * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rho_lower, b->s_rho + off + nx, nx * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_upper, b->s_cnt + off, nx * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_lower, b->s_cnt + off + nx, nx * sizeof(long long), hipMemcpyDeviceToHost));
    memcpy(j_upper, b->surf_rows.data() + off, nx * sizeof(int32_t));
    memcpy(j_lower, b->surf_rows.data() + off + nx, nx * sizeof(int32_t));
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// momentum exchange
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_mex(wtp_batch *b, const double *xref, const double *yref)
{
    WT_TRY(check_batch(b));
    if (!xref || !yref) return fail(WT_ERR_ARG, "xref or yref is null");
    const bool first = !b->xforces.allocated();
    WT_TRY(set_ref_points(b, xref, yref, &b->x_ref));
    const size_t B = (size_t)b->members;
    WT_TRY(alloc_all({{(void **)&b->x_win, B * 2 * sizeof(int32_t)}, {(void **)&b->x_col, B * b->nx * sizeof(MexPartial)},
                      {(void **)&b->x_tickets, B * kTicketStride * sizeof(unsigned int)}}, "momentum-exchange buffers"));
    WT_TRY(b->xforces.alloc(4, (size_t)b->cap, B, "momentum-exchange history"));
    HIP_TRY(hipMemcpy(b->x_win, b->mex_win.data(), B * 2 * sizeof(int32_t), hipMemcpyHostToDevice));     // (the stream is idle)
    HIP_TRY(hipMemsetAsync(b->x_tickets, 0, B * kTicketStride * sizeof(unsigned int), b->st));
    // rows sampled before this call hold no Mz about these points; those before the first call hold nothing at all
    WT_TRY(b->xforces.fill(first ? 0xFu : 1u << 2, b->st));
    b->mex = true;
    return WT_OK;
}

static int check_mex(const wtp_batch *b)
{
    if (!b->mex) return fail(WT_ERR_STATE, "the momentum exchange is not enabled (wtp_enable_mex)");
    return WT_OK;
}

extern "C" int wtp_history_mex(wtp_batch *b, int first, int count, double *fx, double *fy, double *mz, int64_t *links)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_rows(b, first, count));
    WT_TRY(check_mex(b));
    return read_rows(b, b->xforces, first, count, {fx, fy, mz, links});
}

extern "C" int wtp_mex(wtp_batch *b, double *fx, double *fy, double *mz, int64_t *links)
{
    WT_TRY(check_batch(b));
    if (!fx || !fy || !mz || !links) return fail(WT_ERR_ARG, "null output");
    WT_TRY(check_mex(b));
    WT_TRY(check_ready(b));
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(with_dtype(b, [&](auto t) { return launch_mex<decltype(t)>(b, b->cap); }));     // the scratch row
    return read_rows(b, b->xforces, b->cap, 1, {fx, fy, mz, links});
}

extern "C" int wtp_clamp_events(wtp_batch *b, int64_t *rho_events, int64_t *u_events)
{
    WT_TRY(check_batch(b));
    if (!rho_events || !u_events) return fail(WT_ERR_ARG, "null output");
    WT_TRY(check_ready(b));
    HIP_TRY(hipSetDevice(b->device));
    ClampPartial *dp = reinterpret_cast<ClampPartial *>(b->partials);     // (B * nb ForcePartials hold B * nb ClampPartials)
    for (int m = 0; m < b->members; m++) {
        with_dtype(b, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_clamp_events<T>, dim3(b->nb), dim3(256), 0, b->st, (const T *)macro_of<T>(b, m),
                               b->mask + (long)m * b->ms.mask, b->g, 0, b->nx, dp + (long)m * b->nb);
        });
        HIP_TRY(hipGetLastError());
    }
    std::vector<ClampPartial> hp((size_t)b->members * b->nb);
    HIP_TRY(hipStreamSynchronize(b->st));
    HIP_TRY(hipMemcpy(hp.data(), dp, hp.size() * sizeof(ClampPartial), hipMemcpyDeviceToHost));
    for (int m = 0; m < b->members; m++) {
        long long nr = 0, nu = 0;
        for (int q = 0; q < b->nb; q++) { nr += hp[(size_t)m * b->nb + q].rho_events; nu += hp[(size_t)m * b->nb + q].u_events; }
        rho_events[m] = nr; u_events[m] = nu;
    }
    return WT_OK;
}

// One plane of the device to [NY][NX] rows of E on the host, through the stage.  `launch(grd, blk, dst)` enqueues the conversion of the
// plane into the stage, dst, as k_cols_to_rows walks it.
template <typename E, typename Launch>
static int read_plane_by(wtp_batch *b, E *host_dst, Launch launch)
{
    const Geom &g = b->g;
    const size_t bytes = (size_t)b->nx * g.ny * sizeof(E);
    WT_TRY(ensure_stage(b, bytes));
    dim3 blk(32, 8), grd((g.ny + 31) / 32, (b->nx + 31) / 32);
    launch(grd, blk, reinterpret_cast<E *>(b->stage));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_dst, b->stage, bytes, hipMemcpyDeviceToHost, b->st));
    HIP_TRY(hipStreamSynchronize(b->st));
    return WT_OK;
}

// One [NX][pitch] plane of the device (y fastest), as it is stored.
template <typename T>
static int read_plane(wtp_batch *b, const T *src_cols, long pitch, T *host_dst)
{
    return read_plane_by<T>(b, host_dst, [&](dim3 grd, dim3 blk, T *dst) {
        hipLaunchKernelGGL(k_cols_to_rows<T>, grd, blk, 0, b->st, src_cols, dst, 0, b->nx, b->g.ny, pitch);
    });
}

static int check_readable(const wtp_batch *b, int member)
{
    WT_TRY(check_member(b, member));
    if (!b->inited) return fail(WT_ERR_STATE, "no state to read");
    return WT_OK;
}

template <typename T>
static int read_f_impl(wtp_batch *b, int member, void *out)
{
    const size_t n = (size_t)b->nx * b->ny;
    for (int k = 0; k < 9; k++)
        WT_TRY(read_plane<T>(b, fptr<T>(b, b->cur, member) + k * b->g.plane + b->g.pitch, b->g.pitch, reinterpret_cast<T *>(out) + k * n));
    return WT_OK;
}

// wtp_read_f of a half batch: Load of every stored population, plane by plane through the stage.
static int read_f_half(wtp_batch *b, int member, float *out)
{
    const Geom &g = b->g;
    const size_t n = (size_t)b->nx * g.ny;
    const half_t *lat = fptr<half_t>(b, b->cur, member);
    for (int k = 0; k < 9; k++)
        WT_TRY(read_plane_by<float>(b, out + k * n, [&](dim3 grd, dim3 blk, float *dst) {
            hipLaunchKernelGGL(k_half_cols_to_rows, grd, blk, 0, b->st, lat + k * g.plane + g.pitch, dst, 0, b->nx, g.ny, g.pitch, half_w(k));
        }));
    return WT_OK;
}

extern "C" int wtp_read_stored(wtp_batch *b, int member, uint16_t *h)
{
    WT_TRY(check_batch(b));
    if (!h) return fail(WT_ERR_ARG, "h is null");
    if (b->storage != WTP_STORE_HALF) return fail(WT_ERR_STATE, "the batch stores its populations natively (wtp_create_stored)");
    WT_TRY(check_readable(b, member));
    HIP_TRY(hipSetDevice(b->device));
    const size_t n = (size_t)b->nx * b->ny;
    for (int k = 0; k < 9; k++)
        WT_TRY(read_plane<uint16_t>(b, fptr<uint16_t>(b, b->cur, member) + k * b->g.plane + b->g.pitch, b->g.pitch, h + k * n));
    return WT_OK;
}

extern "C" int wtp_read_f(wtp_batch *b, int member, void *f_out)
{
    WT_TRY(check_batch(b));
    if (!f_out) return fail(WT_ERR_ARG, "f_out is null");
    WT_TRY(check_readable(b, member));
    HIP_TRY(hipSetDevice(b->device));
    if (b->storage == WTP_STORE_HALF) return read_f_half(b, member, reinterpret_cast<float *>(f_out));
    return with_dtype(b, [&](auto t) { return read_f_impl<decltype(t)>(b, member, f_out); });
}

// ------------------------------------------------------------------------------------------
// state upload and restart (include/wt_polar.h "State upload and restart")
// ------------------------------------------------------------------------------------------
// Nine [NY][NX] planes of the host, E each, to the member's current lattice, plane by plane through the stage: the inverse of
// read_plane.  `launch(k, src)` enqueues the conversion of plane k from the stage, src, to column 0 of the member's plane.  The stream
// runs dry before the first copy (the stage may still feed an earlier conversion; steps already enqueued end before the values land)
// and after every plane (the next copy reuses the stage); steps enqueued afterwards follow in the stream.
template <typename E, typename Launch>
static int write_planes(wtp_batch *b, const E *in, Launch launch)
{
    const size_t n = (size_t)b->nx * b->ny;
    WT_TRY(ensure_stage(b, n * sizeof(E)));
    HIP_TRY(hipStreamSynchronize(b->st));
    for (int k = 0; k < 9; k++) {
        HIP_TRY(hipMemcpyAsync(b->stage, in + k * n, n * sizeof(E), hipMemcpyHostToDevice, b->st));
        launch(k, reinterpret_cast<const E *>(b->stage));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(b->st));
    }
    return WT_OK;
}

// The elements of the host are those of the lattice (T: float, double, or uint16_t for raw halves): stored as given.
template <typename T>
static int write_raw(wtp_batch *b, int member, const void *in)
{
    const Geom &g = b->g;
    const dim3 blk(32, 8), grd((b->nx + 31) / 32, (g.ny + 31) / 32);
    T *lat = fptr<T>(b, b->cur, member);
    return write_planes<T>(b, reinterpret_cast<const T *>(in), [&](int k, const T *src) {
        hipLaunchKernelGGL(k_rows_to_cols<T>, grd, blk, 0, b->st, src, lat + k * g.plane + g.pitch, 0, b->nx, g.ny, g.pitch, (long)b->nx);
    });
}

// wtp_write_f of a half batch: Store of every fp32 value.
static int write_f_half(wtp_batch *b, int member, const float *in)
{
    const Geom &g = b->g;
    const dim3 blk(32, 8), grd((b->nx + 31) / 32, (g.ny + 31) / 32);
    half_t *lat = fptr<half_t>(b, b->cur, member);
    return write_planes<float>(b, in, [&](int k, const float *src) {
        hipLaunchKernelGGL(k_half_rows_to_cols, grd, blk, 0, b->st, src, lat + k * g.plane + g.pitch, 0, b->nx, g.ny, g.pitch, (long)b->nx,
                           half_w(k));
    });
}

// A write fills columns 0 .. NX-1 and rows 0 .. NY-1 of one lattice only: the start call has to have defined the rest.
static int check_writable(const wtp_batch *b, int member)
{
    WT_TRY(check_member(b, member));
    if (!b->inited) return fail(WT_ERR_STATE, "wtp_init_equilibrium has not been called: pad columns and the other lattice hold nothing defined");
    return WT_OK;
}

// What a write changes besides the populations: the macroscopic planes no longer belong to them, and the member's time statistics restart.
static int after_write(wtp_batch *b, int member)
{
    b->macro_stale = true;
    return clear_sums(b, member, 1);
}

extern "C" int wtp_write_f(wtp_batch *b, int member, const void *f_in)
{
    WT_TRY(check_batch(b));
    if (!f_in) return fail(WT_ERR_ARG, "f_in is null");
    WT_TRY(check_writable(b, member));
    HIP_TRY(hipSetDevice(b->device));
    if (b->storage == WTP_STORE_HALF) WT_TRY(write_f_half(b, member, reinterpret_cast<const float *>(f_in)));
    else WT_TRY(with_dtype(b, [&](auto t) { return write_raw<decltype(t)>(b, member, f_in); }));
    return after_write(b, member);
}

extern "C" int wtp_write_stored(wtp_batch *b, int member, const uint16_t *h)
{
    WT_TRY(check_batch(b));
    if (!h) return fail(WT_ERR_ARG, "h is null");
    if (b->storage != WTP_STORE_HALF) return fail(WT_ERR_STATE, "the batch stores its populations natively (wtp_create_stored)");
    WT_TRY(check_writable(b, member));
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(write_raw<uint16_t>(b, member, h));
    return after_write(b, member);
}

extern "C" int wtp_step_count(wtp_batch *b, int64_t *steps)
{
    WT_TRY(check_batch(b));
    if (!steps) return fail(WT_ERR_ARG, "steps is null");
    *steps = b->steps_done;
    return WT_OK;
}

extern "C" int wtp_set_step_count(wtp_batch *b, int64_t steps)
{
    WT_TRY(check_batch(b));
    if (steps < 0) return fail(WT_ERR_ARG, "steps < 0");
    if (!b->h_step.empty() && steps < b->h_step.back())
        return fail(WT_ERR_STATE, "step count %lld is below that of the last history row held (%lld): wtp_clear_history first",
                    (long long)steps, (long long)b->h_step.back());
    b->steps_done = steps;
    return WT_OK;
}

template <typename T>
static int read_macro_impl(wtp_batch *b, int member, void *rho, void *ux, void *uy)
{
    const long mp = (long)b->g.nxl * b->g.pitch;
    const T *m = macro_of<T>(b, member);
    void *dst[3] = {rho, ux, uy};
    for (int a = 0; a < 3; a++)
        if (dst[a]) WT_TRY(read_plane<T>(b, m + a * mp, b->g.pitch, reinterpret_cast<T *>(dst[a])));
    return WT_OK;
}

extern "C" int wtp_read_macro(wtp_batch *b, int member, void *rho, void *ux, void *uy)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_readable(b, member));
    WT_TRY(check_macro(b));
    HIP_TRY(hipSetDevice(b->device));
    return with_dtype(b, [&](auto t) { return read_macro_impl<decltype(t)>(b, member, rho, ux, uy); });
}

// ------------------------------------------------------------------------------------------
// mean fields
// ------------------------------------------------------------------------------------------
extern "C" int wtp_enable_mean(wtp_batch *b)
{
    WT_TRY(check_batch(b));
    HIP_TRY(hipSetDevice(b->device));
    if (!b->m_sums) {
        const size_t B = (size_t)b->members;
        const int pitch = (b->ny + WTP_MEAN_ROWS - 1) / WTP_MEAN_ROWS * WTP_MEAN_ROWS;
        const long stride = member_stride((size_t)kMeanPlanes * b->nx * pitch * sizeof(double), sizeof(double));
        WT_TRY(alloc_all({{(void **)&b->m_sums, B * (size_t)stride * sizeof(double)}, {(void **)&b->m_cnt, B * sizeof(long long)}},
                         "mean-field sums"));        // (on a failure the batch goes on without the read-out)
        b->m_stride = stride; b->m_pitch = pitch;
    }
    WT_TRY(zero_mean_sums(b, 0, b->members));
    b->mean = true;
    return WT_OK;
}

extern "C" int wtp_mean_sums(wtp_batch *b, int member, int64_t *n, double *rho, double *ux, double *uy, double *rho2, double *ux2,
                             double *uy2, double *uxuy)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_member(b, member));
    if (!b->mean) return fail(WT_ERR_STATE, "the mean fields are not enabled (wtp_enable_mean)");
    HIP_TRY(hipSetDevice(b->device));
    double *dst[kMeanPlanes] = {rho, ux, uy, rho2, ux2, uy2, uxuy};
    const double *src = b->m_sums + (size_t)member * b->m_stride;
    for (int k = 0; k < kMeanPlanes; k++)
        if (dst[k]) WT_TRY(read_plane<double>(b, src + (size_t)k * b->nx * b->m_pitch, b->m_pitch, dst[k]));
    if (n) {
        static_assert(sizeof(int64_t) == sizeof(long long), "the count is 8 bytes");
        HIP_TRY(hipStreamSynchronize(b->st));
        HIP_TRY(hipMemcpy(n, b->m_cnt + member, sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    return WT_OK;
}

// ------------------------------------------------------------------------------------------
// probe points (include/wt_polar.h "Probe points")
// ------------------------------------------------------------------------------------------
static void free_probes(wtp_batch *b)
{
    for (void *p : {(void *)b->pb_off, (void *)b->pb_w, (void *)b->pb_sums, (void *)b->pb_cnt, (void *)b->pb_row}) if (p) (void)hipFree(p);
    b->pb_off = nullptr; b->pb_w = nullptr; b->pb_sums = nullptr; b->pb_cnt = nullptr; b->pb_row = nullptr;
    b->pb_n = 0;
    b->probes = false;
}

extern "C" int wtp_enable_probes(wtp_batch *b, int npoints)
{
    WT_TRY(check_batch(b));
    if (npoints < 0 || npoints > WTP_MAX_PROBES) return fail(WT_ERR_ARG, "npoints must be in [0, %d] (got %d)", WTP_MAX_PROBES, npoints);
    HIP_TRY(hipSetDevice(b->device));
    if (npoints == 0) {
        HIP_TRY(hipStreamSynchronize(b->st));    // samples already enqueued still add to the sums
        free_probes(b);
        return WT_OK;
    }
    const size_t B = (size_t)b->members, P = (size_t)npoints;
    if (npoints != b->pb_n) {                    // another count: new buffers first, so that a failure leaves the batch as it was
        void *off = nullptr, *w = nullptr, *sums = nullptr, *cnt = nullptr, *row = nullptr;
        HIP_TRY(hipStreamSynchronize(b->st));    // samples already enqueued read and write the previous buffers
        WT_TRY(alloc_all({{&off, B * P * sizeof(long long)}, {&w, B * 4 * P * sizeof(double)}, {&sums, B * 3 * P * sizeof(double)},
                          {&cnt, B * sizeof(long long)}, {&row, 3 * P * sizeof(double)}}, "probe tables and sums"));
        free_probes(b);
        b->pb_off = (long long *)off; b->pb_w = (double *)w; b->pb_sums = (double *)sums; b->pb_cnt = (long long *)cnt; b->pb_row = (double *)row;
        b->pb_n = npoints;
    }
    HIP_TRY(hipMemsetAsync(b->pb_off, 0xFF, B * P * sizeof(long long), b->st));      // -1: every point inactive (behind the samples already enqueued)
    HIP_TRY(hipMemsetAsync(b->pb_w, 0, B * 4 * P * sizeof(double), b->st));
    b->probes = true;
    return zero_probe_sums(b, 0, b->members);
}

// The tables of `n` points: off[n] and w[4][n] (k_probe_batch) from x[n], y[n] by the weight rule of include/wt_polar.h, in double, one
// rounding per operation.  False where a point is neither valid nor inactive; *bad is then its index.
static bool probe_tables(const wtp_batch *b, const double *x, const double *y, size_t n, long long *off, double *w, size_t *bad)
{
    const double xmax = (double)b->nx - 0.5, ymax = (double)b->ny - 0.5;
    for (size_t p = 0; p < n; p++) {
        if (std::isnan(x[p])) {                  // inactive: y is not read
            off[p] = -1;
            w[p] = 0.0; w[n + p] = 0.0; w[2 * n + p] = 0.0; w[3 * n + p] = 0.0;
            continue;
        }
        if (!(x[p] >= 0.5 && x[p] <= xmax && y[p] >= 0.5 && y[p] <= ymax)) { *bad = p; return false; }       // (false for a NaN y)
        const double gx = x[p] - 0.5, gy = y[p] - 0.5;
        const int i0 = std::min(std::max((int)std::floor(gx), 0), b->nx - 2), j0 = std::min(std::max((int)std::floor(gy), 0), b->ny - 2);
        const double tx = gx - (double)i0, sx = 1.0 - tx, ty = gy - (double)j0, sy = 1.0 - ty;
        off[p] = (long long)i0 * b->g.pitch + j0;
        w[p] = sx * sy; w[n + p] = tx * sy; w[2 * n + p] = sx * ty; w[3 * n + p] = tx * ty;
    }
    return true;
}

static int check_probes(const wtp_batch *b)
{
    if (!b->probes) return fail(WT_ERR_STATE, "the probe points are not enabled (wtp_enable_probes)");
    return WT_OK;
}

extern "C" int wtp_set_probes(wtp_batch *b, int first, int count, const double *x, const double *y)
{
    WT_TRY(check_batch(b));
    if (!x || !y) return fail(WT_ERR_ARG, "x or y is null");
    WT_TRY(check_members(b, first, count));
    WT_TRY(check_probes(b));
    const size_t P = (size_t)b->pb_n;
    std::vector<long long> off((size_t)count * P);
    std::vector<double> w((size_t)count * 4 * P);
    for (size_t k = 0; k < (size_t)count; k++) {
        size_t bad = 0;
        if (!probe_tables(b, x + k * P, y + k * P, P, off.data() + k * P, w.data() + k * 4 * P, &bad))
            return fail(WT_ERR_ARG, "point %zu of member %d, (%g, %g), lies outside [0.5, %g] x [0.5, %g] and is not inactive (x = NaN)", bad,
                        first + (int)k, x[k * P + bad], y[k * P + bad], (double)b->nx - 0.5, (double)b->ny - 0.5);
    }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));        // samples already enqueued read the previous points
    HIP_TRY(hipMemcpy(b->pb_off + (size_t)first * P, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b->pb_w + (size_t)first * 4 * P, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
    return zero_probe_sums(b, first, count);
}

// Three [P] arrays of the device, one behind the other from `src`, to the destinations that are not null.
static int read_probe_values(const wtp_batch *b, const double *src, double *rho, double *ux, double *uy)
{
    const size_t P = (size_t)b->pb_n;
    double *const dst[3] = {rho, ux, uy};
    for (int a = 0; a < 3; a++)
        if (dst[a]) HIP_TRY(hipMemcpy(dst[a], src + (size_t)a * P, P * sizeof(double), hipMemcpyDeviceToHost));
    return WT_OK;
}

extern "C" int wtp_probe_sums(wtp_batch *b, int member, int64_t *n, double *rho, double *ux, double *uy)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_member(b, member));
    WT_TRY(check_probes(b));
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->st));
    WT_TRY(read_probe_values(b, b->pb_sums + (size_t)member * 3 * b->pb_n, rho, ux, uy));
    if (n) HIP_TRY(hipMemcpy(n, b->pb_cnt + member, sizeof(int64_t), hipMemcpyDeviceToHost));
    return WT_OK;
}

// One member's points sampled on the last emitted state into the scratch row: a grid of one row with the member's planes and tables.
template <typename T>
static int launch_probe_sample(wtp_batch *b, int member)
{
    const size_t P = (size_t)b->pb_n;
    hipLaunchKernelGGL((k_probe_batch<T, false>), dim3((unsigned)((b->pb_n + 255) / 256), 1u), dim3(256), 0, b->st,
                       (const T *)macro_of<T>(b, member), b->g, b->ms, b->pb_n, (const long long *)(b->pb_off + (size_t)member * P),
                       (const double *)(b->pb_w + (size_t)member * 4 * P), b->pb_row, (long long *)nullptr);
    HIP_TRY(hipGetLastError());
    return WT_OK;
}

extern "C" int wtp_probe_sample(wtp_batch *b, int member, double *rho, double *ux, double *uy)
{
    WT_TRY(check_batch(b));
    WT_TRY(check_member(b, member));
    WT_TRY(check_probes(b));
    WT_TRY(check_ready(b));
    WT_TRY(check_macro(b));
    HIP_TRY(hipSetDevice(b->device));
    WT_TRY(with_dtype(b, [&](auto t) { return launch_probe_sample<decltype(t)>(b, member); }));
    HIP_TRY(hipStreamSynchronize(b->st));
    return read_probe_values(b, b->pb_row, rho, ux, uy);
}
