/*
 * negf_layered_channels.h -- transmission eigenchannels of layered devices: the second header of libnegf_hip.so's C ABI.
 *
 * Everything of negf.h holds here as well: its conventions (interleaved complex128, row-major; host and "*_dev"
 * pointers; the caller owns every buffer; return 0 = ok, < 0 = argument / runtime error, > 0 = numerical condition),
 * its error codes, its context and the stream contract of its device-resident calls.  A layered system and its
 * terminals are made with negf_layered_create / negf_layered_terminal_* of negf.h.  gaunegf_amd/_lib.py binds the
 * symbols below in a table of their own (SIGNATURES_LAYERED_CHANNELS), gaunegf_amd/layered.py re-exposes them as
 * calculate_eigenchannels_layered, channel_count_layered, eigvalsh_wide and set_channel_algo.
 *
 * Definition (negf_transmission_channels' on the corner block of G).  For terminals a, b on OPPOSITE end layers with
 * orbital lists I_a, I_b (K_a, K_b) inside their layers:
 *   Gamma_t = i (Sigma_t - Sigma_t^H) on the terminal's K_t orbitals,   G_ab = G[I_a, I_b], cut from the corner block
 *   (G_{0,L-1} when a sits on layer 0, G_{L-1,0} when on the last layer),
 *   Gamma_a = L L^H by PIVOTED Cholesky, truncated where the largest remaining diagonal is <= 1e-14 max diag Gamma_a or
 *   not positive (rank r),   B = G_ab Gamma_b G_ab^H,   T_n = the eigenvalues of H = L^H B L (r x r).
 * When K_b < K_a the mirror form factors Gamma_b instead (B = G_ab^H Gamma_a G_ab): the eigenproblem lives on the
 * smaller list.  T_n are the eigenvalues of t^H t; sum_n T_n = negf_layered_transmission(term_a, term_b) up to rounding
 * and the cut.  Values only: scattering states are not served on layered systems.
 *
 * Kernels.  min(K_a, K_b) <= 96 takes the kernels of negf_transmission_channels (the matrix in one compute unit's LDS),
 * 96 < min(K_a, K_b) <= 512 the wide kernels: a left-looking pivoted Cholesky and a Householder tridiagonalisation
 * followed by bisection with Sturm counts, one workgroup per matrix, the matrix in a workgroup-private slice of global
 * memory.  Every sum has a fixed order: results are bitwise the same from run to run and do not depend on
 * negf_set_batch; scaling E, F and Sigma by a power of two leaves T_n bitwise unchanged.
 *
 * Work areas (what negf_layered_workspace_bytes reports after such a call): the 10 matrices of the largest layer per
 * energy in flight of a corner sweep; per energy in flight Gamma_a, Gamma_b (K_a^2 + K_b^2), G_ab, Z, W (3 K_a K_b), H
 * (K_s^2, K_s = min(K_a, K_b)) and, for the wide eigensolver, its K_s^2 copy of H; L^H (K_s^2) and its rank once per
 * call for a const terminal, per energy in flight otherwise; in the host form the [m][nchan] staging of the result.
 */
#ifndef NEGF_LAYERED_CHANNELS_H
#define NEGF_LAYERED_CHANNELS_H

#include "negf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* min(K_a, K_b): the number of channels of (term_a, term_b).  NEGF_EINVAL: unknown handle or terminal, both terminals
 * on the same end (as negf_layered_transmission), or min(K_a, K_b) > 512. */
int negf_layered_channel_count(negf_ctx* ctx, int handle, int term_a, int term_b, int* nchan);

/* T_chan [m][nchan]: the min(nchan, count) largest channels per energy in DESCENDING order, not clamped; exact zeros at
 * or beyond the rank and in columns >= count.  All three kinds of terminal are served: a const terminal is factored
 * once per call, chain and blocks terminals per energy; more energies than a blocks terminal holds is NEGF_EINVAL before
 * anything is launched (as nchan < 1 and the refusals of negf_layered_channel_count).  info [m] or NULL: as
 * negf_layered_transmission (a singular layer gives a NaN row -- every one of its nchan columns --, the 1-based pivot
 * column numbered in the whole system and NEGF_ESINGULAR), and -1 where the eigensolver met a non-finite H (NaN row,
 * NEGF_ESINGULAR as well; -2, the Jacobi kernel's "not converged", can occur for K_s <= 96 only).  The other energies
 * are unaffected.  The _dev form follows the stream contract of negf.h: it overwrites T_chan_dev and waits for the
 * host where negf_layered_transmission_dev does (a buffer that has to grow), nowhere else. */
int negf_layered_transmission_channels(negf_ctx* ctx, int handle, int term_a, int term_b, int m, const double* E_c128,
                                       int nchan, double* T_chan, int* info);
int negf_layered_transmission_channels_dev(negf_ctx* ctx, int handle, int term_a, int term_b, int m, const double* E_dev,
                                           int nchan, double* T_chan_dev);

/* Diagnostic, like negf_zgemm_batched: the WIDE eigenvalue kernel alone at any 1 <= K <= 512 (NEGF_EINVAL beyond).
 * negf_eigvalsh_batched's semantics: m Hermitian K x K matrices read from their lower triangles (imaginary parts of the
 * diagonal ignored), A_c128 [m][K][K], w [m][K] ascending; info [m] or NULL: 0, 1 = non-finite input (NaN row);
 * NEGF_ESINGULAR when any info is nonzero.  (The kernel has no convergence failure: info 2 does not occur.) */
int negf_eigvalsh_wide_batched(negf_ctx* ctx, int K, int m, const double* A_c128, double* w, int* info);

/* Which kernels negf_layered_transmission_channels runs: 0 = by size (default: K_s <= 96 the LDS kernels, above that the
 * wide ones), 1 = the wide kernels at every K_s (tests).  Acts on the layered channel call only; other values:
 * NEGF_EINVAL. */
int negf_set_channel_algo(negf_ctx* ctx, int algo);

#ifdef __cplusplus
}
#endif
#endif /* NEGF_LAYERED_CHANNELS_H */
