/*
 * wt_polar.h — C-ABI of libwtpolar.so: batched angle-of-attack sweeps.
 *
 * A batch holds B independent wind tunnels ("members") of one lattice size and
 * dtype on one GPU.  Each member has its own mask, tau and U0; all members
 * advance together, one kernel launch per step for the whole batch.  Every
 * member's state is bit-identical to a libwindtunnel handle (wt_create) given
 * the same mask, tau, U0 and step sequence.  Lift, drag and separation are
 * reduced on the device after sampled steps into a history buffer that the
 * host reads once (wtp_history); every sample equals what wt_forces returns on
 * a single handle at that step, bit for bit.
 *
 * Conventions are those of windtunnel.h: every function returns 0 (WT_OK) or a
 * negative wt_status, the calling thread's last failure is wtp_last_error(),
 * nothing aborts across the boundary, the caller owns every host buffer.
 * Host arrays are C-contiguous; masks are [count][NY][NX] bytes (non-zero =
 * solid), populations [9][NY][NX], macroscopic fields [NY][NX], all of the
 * batch's dtype.  Per-member arrays are [B].  A batch is driven by one host
 * thread at a time.  There is no CPU fallback.
 */
#ifndef WT_POLAR_H
#define WT_POLAR_H

#include <stdint.h>
#include "windtunnel.h"      /* wt_status, wt_dtype */

#if defined(__GNUC__)
#define WTP_API __attribute__((visibility("default")))
#else
#define WTP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wtp_batch wtp_batch;

#define WTP_MAX_MEMBERS 1024

/* nx, ny >= 3 (as wt_create), 1 <= members <= WTP_MAX_MEMBERS, history_cap >= 0 samples, dtype WT_F32 or WT_F64.
 * Bad arguments fail with WT_ERR_ARG before any device call. */
WTP_API int wtp_create(int nx, int ny, int dtype, int members, int history_cap, int device, wtp_batch **out);
WTP_API int wtp_destroy(wtp_batch *b);
WTP_API const char *wtp_last_error(void);
WTP_API const char *wtp_version(void);

/* Masks of members [first, first+count): [count][NY][NX].  The flow state is kept, as by wt_set_mask. */
WTP_API int wtp_set_masks(wtp_batch *b, int first, int count, const uint8_t *masks);
/* Uniform equilibrium at u0[m] for every member (as wt_init_equilibrium); the step count restarts at 0 and the history is cleared. */
WTP_API int wtp_init_equilibrium(wtp_batch *b, const double *u0);
/* Enqueue nsteps steps of every member with tau[m], u0[m].  The last step of the call emits (rho, ux, uy), as wt_step.
 * sample_every > 0: every step whose count since wtp_init_equilibrium is a multiple of sample_every also emits and is
 * followed by the force reduction of every member into the next history row.  A call whose samples would overflow the
 * history fails with WT_ERR_STATE before anything is enqueued. */
WTP_API int wtp_step(wtp_batch *b, int nsteps, const double *tau, const double *u0, int sample_every);
/* Rows [first, first+count) of the history: step[count] (the step count of the row), fx / fy / surf / rev [count][B]
 * (wt_forces' four values per member).  Any output pointer may be NULL.  Returns the number of rows held (>= 0). */
WTP_API int wtp_history(wtp_batch *b, int first, int count, int64_t *step, double *fx, double *fy, int64_t *surf, int64_t *rev);
WTP_API int wtp_clear_history(wtp_batch *b);
/* wt_forces of every member on the last emitted state: [B] each. */
WTP_API int wtp_forces(wtp_batch *b, double *fx, double *fy, int64_t *surf, int64_t *rev);
/* wt_clamp_events of every member: [B] each. */
WTP_API int wtp_clamp_events(wtp_batch *b, int64_t *rho_events, int64_t *u_events);
/* One member's populations [9][NY][NX] / macroscopic fields [NY][NX] (any of rho, ux, uy may be NULL). */
WTP_API int wtp_read_f(wtp_batch *b, int member, void *f_out);
WTP_API int wtp_read_macro(wtp_batch *b, int member, void *rho, void *ux, void *uy);
/* Wait for the enqueued work. */
WTP_API int wtp_sync(wtp_batch *b);

#ifdef __cplusplus
}
#endif

#endif /* WT_POLAR_H */
