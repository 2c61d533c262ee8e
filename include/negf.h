/*
 * negf.h -- C ABI of libnegf_hip.so, the MI355X (gfx950) NEGF energy-grid engine.
 *
 * The reference (wliverno/GauNEGF) is pure Python and has no FFI of its own; the
 * seams this library sits behind are its Python call sites.  Each entry point
 * below names the reference function it replaces (file:line in the reference
 * checkout).  gaunegf_amd/_lib.py binds exactly these symbols with ctypes and
 * gaunegf_amd/{integrate,transport,density,surfG1D,surfGBethe}.py re-expose them
 * under the reference's own names (GrInt, GrLessInt, calculate_transmission ...).
 *
 * Conventions
 *   - complex128 arrays are interleaved (re,im) doubles, row-major (C order), i.e.
 *     the memory of a C-contiguous numpy complex128 array.
 *   - "host" pointers are ordinary CPU memory; "*_dev" pointers are HIP device
 *     memory on the context's GPU (e.g. torch.Tensor.data_ptr()).
 *   - the caller owns every buffer; nothing is retained after a call returns,
 *     except data copied by negf_set_system / negf_sigma_* into the context.
 *   - return 0 = ok, <0 = argument / runtime error, >0 = numerical condition
 *     (NEGF_ESINGULAR: at least one energy hit an exactly zero pivot or a NaN
 *     column; info[k] holds the 1-based pivot column for energy k, LAPACK style,
 *     and G(E_k) is NaN-filled by the blocked kernels -- numpy/jax solve would
 *     return inf/NaN there as well; the other energies are unaffected).  A self-energy
 *     fixed point that stops at its iteration cap is NOT an error (the reference
 *     stops silently too, surfG1D.py:290-293); it is reported via converged[].
 *   - one negf_ctx per (process, GPU); calls are blocking unless noted and the
 *     context is not thread-safe (mirrors FORCE_SYNCHRONOUS, integrate.py:56).
 *   - there is NO CPU fallback: negf_create fails with NEGF_ENODEV without a GPU.
 */
#ifndef NEGF_H
#define NEGF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct negf_ctx negf_ctx;

#define NEGF_OK          0
#define NEGF_EINVAL     (-1)
#define NEGF_ENOMEM     (-2)
#define NEGF_EHIP       (-3)
#define NEGF_ENODEV     (-4)
#define NEGF_ESTATE     (-5)
#define NEGF_ESINGULAR    1

/* contact selector for "use the total self-energy" (Python ind=None,
 * integrate.py:201-204).  Other negative values index from the end like Python
 * (ind=-1 is the last contact, scfE.py:441,444). */
#define NEGF_IND_TOTAL  (-1000)
/* selector of the RETARDED form of negf_population / negf_projected_dos (no contact: the quantity is built on G itself);
 * no other entry point accepts it */
#define NEGF_IND_RETARDED (-2000)

/* spin layouts of transport.py:193-271 */
#define NEGF_SPIN_RESTRICTED 0   /* 'r'                         */
#define NEGF_SPIN_BLOCK      1   /* 'u' / 'ro' (and 'g' after the host permutes spinor -> block form) */

/* ---------------------------------------------------------------- lifetime */
int         negf_device_count(void);                 /* 0 when no GPU / no driver */
int         negf_create(negf_ctx** out, int device);
void        negf_destroy(negf_ctx* ctx);
const char* negf_strerror(int code);
const char* negf_version(void);
/* Launch everything on this hipStream_t (NULL = the default stream).  A context has ONE stream at a time: its work
 * areas are reused from call to call in that stream's order.  When the stream changes, the new one is ordered behind
 * the old one ON THE DEVICE (an event recorded on the old stream, waited for by the new one): work queued before the
 * switch finishes before anything queued after it starts, and the host does not wait.  The old stream must still
 * exist at the call.  Setting the stream that is already set does nothing and costs nothing.  Work the CALLER has on
 * other streams is the caller's to order (events), as with any stream-ordered library; two contexts are independent
 * of each other, whatever their streams. */
int         negf_set_stream(negf_ctx* ctx, void* hip_stream);
/* energies processed per sweep of the workspace (0 = choose from n and free HBM);
 * replaces MAX_VMAP_MEMORY_GB batching, integrate.py:55,100-142.
 * batch = b > 0 is a LIMIT, for memory as well (what a caller who shares a device sets it for): from the next call on no
 * dense call sweeps more than b energies, and the workspace -- three n x n matrices per energy, the bulk of what a
 * context holds -- holds no more than b of them.  (What shrinks is that workspace with its pivot, site and Sigma-block
 * staging; the smaller per-sweep areas of single entry points -- channels, transmission matrix, probes, segment sums --
 * only grow, and keep the size of the largest sweep they have served until the system's dimension changes.)
 * A workspace in place that is larger than b is released and rebuilt at min(b, m) for the call's m energies; one that is
 * not larger is kept, or grown to min(b, m) where the grid asks for it.  negf_transmission needs two energies' worth
 * and sweeps half of what stands: b = 1 gives a workspace of 2 and sweeps of 1, b = 6 sweeps of 3.  batch = 0 lifts the
 * limit: the workspace then only grows, to the grid (twice the grid once a transmission has run on the context) within
 * the memory budget.  negf_get_batch and negf_workspace_bytes report the workspace in place.
 * Per-energy results, and the sums whose comment below says so, do not depend on the limit AS LONG AS the inverse takes the
 * same kernels for the sweeps compared: "do not depend on negf_set_batch" below is to be read with that condition.  The
 * inverse chooses its kernels from n and the number of energies in a sweep (negf_inverse_plan reports the choice); two
 * sweep sizes with different plans give G(E) that differ in rounding, each within the accuracy bound of the inverse, not
 * the same bits.  The other weighted sums (negf_gr_int, negf_gless_int, their _seg forms, negf_gr_int_probes,
 * negf_gr_int_refine) add 32 energies of a SWEEP at a time: their bits depend on the sweeps, within the summation bound
 * of DESIGN.md's accumulate section. */
int         negf_set_batch(negf_ctx* ctx, int batch);
int         negf_get_batch(negf_ctx* ctx);

/* F,S of the device region: the (F, S) arguments of GrInt/GrLessInt
 * (integrate.py:146,177) and of the transport kernels (transport.py:150-190).
 * Both n*n complex128 (a real F is passed with zero imaginary parts). */
int negf_set_system(negf_ctx* ctx, int n, const double* F_c128, const double* S_c128);

/* 64-bit checksum of a host buffer (no context, no GPU; large buffers on up to 8 threads): what the front end's caches use
 * to notice that a caller changed a matrix in place between two entry points (gaunegf_amd/engine.py fingerprint). */
unsigned long long negf_hash_bytes(const void* data, unsigned long long bytes);

/* The same with a caller's key (0: none).  Equal nonzero keys VOUCH that (F, S) are bitwise the matrices handed over with
 * that key before: a resident system with the key is selected without comparing 2 x 16 n^2 bytes on the host (a front end
 * that keeps private, immutable complex copies of the caller's matrices numbers them -- gaunegf_amd/engine.py; an entry
 * point of a per-GPU share of BASELINE C5 spent 4 ms of its 30 comparing).  An unknown key falls back to the comparison. */
int negf_set_system_keyed(negf_ctx* ctx, int n, const double* F_c128, const double* S_c128, unsigned long long key);

/* ------------------------------------------------- self-energy providers
 * A provider is the device-side lowering of the reference's duck-typed ``g``
 * object (.sigma(E,i) / .sigmaTot(E)).  Handles are small
 * non-negative ints owned by the context. */

/* energy-independent Sigma: surfGTester.py:94-132 / SigmaCalculator static
 * (sig1,sig2), transport.py:77-117.  sigma_c128 = [n_contacts][n][n]; the
 * total is their sum in contact order. */
int negf_sigma_const(negf_ctx* ctx, int n_contacts, const double* sigma_c128, int* handle);

/* 1-D chain decimation provider: surfG1D.py:223-399.  Per contact c the block
 * size nc[c] and orbital indices inds (concatenated), and the nc x nc complex128
 * matrices alpha,Salpha,beta,Sbeta,tau,Stau (concatenated in contact order).
 * eta/conv/relFactor/max_iter default in the reference to ETA=1e-6 (config.py:9),
 * 1e-5 (config.py:15), 0.1 (config.py:16), 2000 (surfG1D.py:265).
 * Pivoting inside the fixed point's inverses (n_c <= 64 kernel): partial pivoting by LAPACK's izamax metric
 * |re| + |im|, compared on the HIGH 32-bit word of the double (sign, exponent, 20 mantissa bits); candidates whose
 * metrics agree to 2^-20 relative count as tied and the lowest row wins, as LAPACK's exact ties do.  (The dense
 * inverses of the hot path compare 36 mantissa bits.)  A different pivot among near-equal candidates changes
 * rounding only: parity with the reference is 1e-10 at a fixed trip count (observed 1e-13).
 * force_iters >= 0 runs exactly that many sweeps (parity at fixed trip count);
 * pass -1 for the reference's data-dependent stopping rule. */
int negf_sigma_chain1d(negf_ctx* ctx, int n_contacts, const int* nc, const int* inds,
                       const double* alpha, const double* Salpha,
                       const double* beta, const double* Sbeta,
                       const double* tau, const double* Stau,
                       double eta, double conv, double relFactor, int max_iter,
                       int force_iters, int* handle);

/* 1-D chain provider with the renormalisation-decimation ("doubling", Lopez Sancho - Rubio) solver: a CHAIN1D provider
 * like negf_sigma_chain1d's -- same arguments, same kind, served by every entry point that serves that one -- whose
 * surface Green's function is NOT found by the reference's relaxed loop (surfG1D.py:223-295:
 * g <- 0.1 inv(A - B g B^H) + 0.9 g until the relative change is <= 1e-5 or 2000 sweeps have run) but by
 *     es = e = A,  a = B,  b = B^H          (A = (E + i eta) Salpha - alpha, B = (E + i eta) Sbeta - beta; b is taken as a
 *                                            matrix, so it conjugates the complex energy as surfG1D.py:262 does)
 *     step:  G = inv(e);  P = a G;  Q = b G;  D = P b
 *            es <- es - D;   e <- e - D - Q a;   a <- P a;   b <- Q b;   steps += 1
 *     g = inv(es);   Sigma = t g t^H,  t = E Stau - tau
 * Stop rule: after the step in which  max |D_ij| <= tol * max |es_ij|  (es already updated; |x| = |re| + |im|, the
 * izamax metric: a relative test, exact under power-of-two scaling), or at max_steps.  tol = 2^-52 means "the
 * correction no longer reaches es"; the Python layer's defaults are tol = 2^-52, max_steps = 64.
 * Step k of the recursion IS iterate 2^k - 1 of the unrelaxed loop g <- inv(A - B g B^H) started from inv(A): the same
 * semi-infinite chain, doubled in length at every step instead of grown by one cell.
 * force_steps >= 0 runs exactly that many steps (0: g = inv(A)); -1 the stop rule.  negf_last_iters reports the steps
 * and converged = 0 for a unit that reached max_steps (it returns what it has) or met a zero pivot / non-finite input
 * (a NaN block).  Inverses for n_c <= 64 use the pivoting rule described at negf_sigma_chain1d.  The g(E) cache keys
 * on the solver and on tol / max_steps / force_steps: the two solvers never serve each other's entries. */
int negf_sigma_chain1d_rd(negf_ctx* ctx, int n_contacts, const int* nc, const int* inds,
                          const double* alpha, const double* Salpha,
                          const double* beta, const double* Sbeta,
                          const double* tau, const double* Stau,
                          double eta, double tol, int max_steps, int force_steps, int* handle);

/* Bethe-lattice provider: surfGBethe.py:479-575, 958-1108.  Per contact: onsite
 * H [9][9] and the 12 direction matrices S,V [12][9][9] (all float64), the list
 * of contact atoms (orbital indices [n_atoms][9], concatenated over contacts) and
 * for every atom its attached-direction list (n_nb[atom] entries of nb_dirs,
 * concatenated).  xi_c128 = S^{1/2} [n][n] or NULL (applied as Xi sig Xi when the
 * .bethe file has Ssss == 0, surfGBethe.py:530-533).  mix=0.5, max_iter=1000 in
 * the reference (:958,:998). */
int negf_sigma_bethe(negf_ctx* ctx, int n_contacts, const int* n_atoms,
                     const int* atom_orbs, const int* n_nb, const int* nb_dirs,
                     const double* H, const double* Slist, const double* Vlist,
                     const double* xi_c128,
                     double eta, double conv, double mix, int max_iter,
                     int force_iters, int* handle);

/* The single-atom Bethe lattice itself: surfGBAt.sigmaK (which = 1, out [m][12][9][9],
 * surfGBethe.py:958-1030) or surfGBAt.sigma (which = 2, out [m][9][9][9], :1032-1108).
 * H [9][9], Slist/Vlist [12][9][9] float64.  iters[m]: bulk sweeps (which = 1) or
 * bulk + (surface << 16) (which = 2); converged[m] likewise (bit 0 bulk, bit 1 surface). */
int negf_bethe_raw(negf_ctx* ctx, const double* H, const double* Slist, const double* Vlist,
                   double eta, double conv, double mix, int max_iter, int force_iters,
                   int which, int m, const double* E_c128, double* out_c128,
                   int* iters, int* converged);

/* Sigma evaluated by the caller for exactly the energies of the NEXT integral
 * (arbitrary user ``g`` objects, integrate.py:169,203-204): sigma_tot [m][n][n]
 * and, optionally, the contact Sigma_c used for Gamma [m][n][n] (NULL = use
 * sigma_tot).  n_contacts_c > 1 means sigma_c holds [m][n_contacts_c][n][n].
 * n_contacts_c < 0: sigma_c holds [m][-n_contacts_c][n][n] matrices that ARE the
 * couplings Gamma (used as given instead of i(Sigma_c - Sigma_c^H)); this is how
 * _transmission_kernel_restricted(E,F,S,sigma_total,gamma1,gamma2)
 * (transport.py:150-157), whose gammas are arguments, is served. */
int negf_sigma_precomputed(negf_ctx* ctx, int m, const double* sigma_tot_c128,
                           int n_contacts_c, const double* sigma_c_c128, int* handle);

int negf_sigma_free(negf_ctx* ctx, int handle);

/* Sigma(E) itself: g.sigma(E,i) / g.sigmaTot(E) (surfG1D.py:344-399,
 * surfGBethe.py:479-575).  contact = NEGF_IND_TOTAL or a contact index.
 * sigma_out [m][n][n]; iters / converged are [m][n_contacts] (may be NULL). */
int negf_sigma_eval(negf_ctx* ctx, int handle, int contact, int m, const double* E_c128,
                    double* sigma_out_c128, int* iters, int* converged);

/* ------------------------------------------------------------- the hot path */

/* sum_m w_m G^r(E_m) -- GrInt, integrate.py:146-173 (+ _gr_matrix_ops :67-71,
 * _GInt :84-142).  out [n][n]; info [m] or NULL. */
int negf_gr_int(negf_ctx* ctx, int handle, int m, const double* E_c128,
                const double* w_c128, double* out_c128, int* info);

/* Several GrInt integrals of one system in ONE pass: the m energies are nseg consecutive segments, seg_end[s] = index
 * one past segment s (seg_end[nseg-1] = m), out [nseg][n][n] receives one sum per segment.  Serves the adaptive
 * integrations -- integratePointsAdaptiveANT, density.py:211-273 (nested levels of 2, 6, 18, 54 ... nodes, only the
 * new nodes of a level are evaluated) and the doubling grids of densityReal, :438-484 -- whose first levels are a
 * handful of points each: evaluated level by level they are launch latency, evaluated together they are one launch.
 * Every segment's sum equals negf_gr_int on that segment alone up to summation order. */
int negf_gr_int_seg(negf_ctx* ctx, int handle, int m, const double* E_c128, const double* w_c128,
                    int nseg, const int* seg_end, double* out_c128, int* info);

/* integratePointsAdaptiveANT (density.py:211-273) with the refinement on the device.  The m energies are the NEW nodes of
 * consecutive levels of nint adaptive integrations of one system: nlev[k] levels for integration k, seg_end[s] as above over all
 * sum(nlev) levels (integration after integration), ratio[s] = the nested-weight ratio of level s (density.py:248-252) -- NaN
 * for the first level of an integration (P = that level's sum, no test); an integration whose first ratio is a number continues
 * from P_in[k].  Per level, in the reference's order: new_P = P * ratio; new_P += sum; maxDP = max|new_P - P|; stop when
 * maxDP < tol (density.py:253-268).  P_out [nint][n][n]: the value at the converged level or after the last one; level_out [nint]:
 * index of the converged level within the call or -1 (continue with P_out as P_in); maxdp_out [sum(nlev)] (NaN: level not
 * consumed / first level).  nint <= 64, at most 2048 levels in all. */
int negf_gr_int_refine(negf_ctx* ctx, int handle, int m, const double* E_c128, const double* w_c128, int nint,
                       const int* nlev, const int* seg_end, const double* ratio, double tol, const double* P_in_c128,
                       double* P_out_c128, int* level_out, double* maxdp_out, int* info);

/* ... and the same for GrLessInt: the levels of the adaptive bias-window integral (densityGrid, density.py:605-658). */
int negf_gless_int_seg(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, const double* w_c128,
                       int nseg, const int* seg_end, double* out_c128, int* info);

/* sum_m w_m G Gamma_c G^H -- GrLessInt, integrate.py:177-208 (+ :74-82). */
int negf_gless_int(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128,
                   const double* w_c128, double* out_c128, int* info);

/* every G^r(E_m) [m][n][n]; used by parity tests and by callers that need G(E). */
int negf_gr_batch(negf_ctx* ctx, int handle, int m, const double* E_c128,
                  double* G_out_c128, int* info);

/* Re Tr[Gamma_L G Gamma_R G^H] per energy -- _transmission_kernel_restricted /
 * _transmission_kernel_spin_block, transport.py:150-181.  T [m]; Tspin [m][4]
 * (uu,ud,du,dd) or NULL, required for NEGF_SPIN_BLOCK. */
int negf_transmission(negf_ctx* ctx, int handle, int contact_L, int contact_R,
                      int spin_mode, int m, const double* E_c128,
                      double* T, double* Tspin, int* info);

/* -Im diag G / pi and its sum -- _dos_kernel transport.py:183-190,
 * _compute_dos_at_energy density.py:49-54.  dos_site [m][n] or NULL. */
int negf_dos(negf_ctx* ctx, int handle, int m, const double* E_c128,
             double* dos_total, double* dos_site, int* info);

/* ----------------------------------------------- device-resident variants
 * Same operations with the energy grid, weights and result already in HBM on
 * the context's GPU (used by bench.py and by the multi-GPU driver, which
 * all-reduces out_dev with RCCL through torch.distributed).  Asynchronous on
 * the context's stream; negf_sync waits.  negf_last_info copies the per-energy
 * info of the last *_dev call.
 *
 * The stream contract of every *_dev entry point in this header (these, the layered ones and the later sections'):
 *   - E_dev, w_dev and every other device input are READ IN STREAM ORDER: work the caller queued on the context's
 *     stream before the call (copies into E_dev, kernels that produce the weights) is seen, whether or not it has
 *     finished when the call returns.  Host arrays (seg_end, probe and group tables) are read before the call returns.
 *   - out_dev / T_dev / ... are OVERWRITTEN: never accumulated into, never read; the caller need not zero them.
 *   - Results are valid IN STREAM ORDER on that stream -- work queued behind the call sees them -- or on the host
 *     after negf_sync (or any other wait for that stream).  negf_last_info and negf_last_iters wait themselves.
 *   - Calls on one context may follow each other without a wait in between: they share the context's work areas in
 *     stream order (also across negf_set_stream, see there).
 *   - The call itself does not wait for the stream, EXCEPT
 *       * a call that has to grow a buffer of the context (the first call of a shape, a larger grid, a larger batch):
 *         it drains the stream before it frees the old buffer;
 *       * a CHAIN1D provider (and a chain terminal of a layered system) while the g(E) cache is on
 *         (negf_set_chain_cache, on by default): the energies are the cache key, so E_dev is downloaded -- one copy
 *         and one wait per launch of the chain kernels, in stream order like every other read;
 *       * a CHAIN1D provider with a free-running fixed point (force_iters < 0) whose record of sweep counts has to grow;
 *       * an entry point that stages host tables on the device uploads them with a wait on every call: the probe and
 *         group tables of the transmission-matrix, dephasing, bond and population calls, and the selected terminals'
 *         orbital lists of negf_layered_gless_int_dev and negf_layered_contact_dos_dev.
 *     With the cache off, CONST / PRECOMPUTED / BETHE providers and CHAIN1D at a fixed sweep count, a warm call of
 *     negf_gr_int_dev, negf_gless_int_dev, negf_gr_int_seg_dev, negf_gless_int_seg_dev, negf_transmission_dev,
 *     negf_layered_gr_int_dev, negf_layered_dos_dev and negf_layered_transmission_dev returns while the stream is
 *     still busy with earlier work.
 *   - A singular energy is no error of a *_dev call: it is reported through negf_last_info (non-zero at that energy). */
int negf_gr_int_dev(negf_ctx* ctx, int handle, int m, const double* E_dev,
                    const double* w_dev, double* out_dev);
int negf_gless_int_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev,
                       const double* w_dev, double* out_dev);
/* negf_gr_int_seg / negf_gless_int_seg with grid, weights and the nseg results [nseg][n][n] in HBM (seg_end stays a host
 * array): several integrals of one system -- contour + real axis of a density step (scfE.py:316-328), the levels of an
 * adaptive integration -- as ONE pass over this rank's shard of all their energies and ONE all-reduce of out_dev. */
int negf_gr_int_seg_dev(negf_ctx* ctx, int handle, int m, const double* E_dev, const double* w_dev,
                        int nseg, const int* seg_end, double* out_dev);
int negf_gless_int_seg_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, const double* w_dev,
                           int nseg, const int* seg_end, double* out_dev);
/* NEGF_SPIN_RESTRICTED writes T_dev [m]; NEGF_SPIN_BLOCK writes Tspin_dev [m][4] only (T_dev is not touched: the
 * total is the sum of the four components, which negf_transmission forms on the host). */
int negf_transmission_dev(negf_ctx* ctx, int handle, int contact_L, int contact_R,
                          int spin_mode, int m, const double* E_dev,
                          double* T_dev, double* Tspin_dev);
int negf_sync(negf_ctx* ctx);
int negf_last_info(negf_ctx* ctx, int m, int* info);
/* sweeps / converged flags of the self-energy fixed points run by the last call
 * ([m][n_contacts] each; the counts the reference's lax.while_loop state carries,
 * surfG1D.py:271-288, surfGBethe.py:1004-1022); zeros / ones for providers without a loop */
int negf_last_iters(negf_ctx* ctx, int handle, int m, int* iters, int* converged);

/* ------------------------------------------ surface Green's function cache
 * The decimation fixed point g(E) of a 1-D chain lead (surfG1D.py:223-295) depends on the lead cell (alpha, Salpha,
 * beta, Sbeta), eta, conv, relFactor, max_iter and E -- not on F and not on the coupling blocks tau (:256-262; setF
 * refreshes tau only, :319-329).  The reference recomputes it inside every vmapped closure (integrate.py:168-171) and
 * twice per energy in GrLessInt (:201-204).  The context keeps the final iterates of the last `max_grids` launches of
 * the n_c <= 64 chain kernel in HBM (n_contacts * n_c^2 * 16 bytes per energy), keyed BITWISE on those inputs and on
 * the energy list of the launch; a launch that finds its key only forms Sigma = t g t^H with the provider's CURRENT
 * tau -- the last pass of the same kernel, so a hit equals a miss bit for bit, sweep counts and flags included.  The
 * key outlives providers: one re-created after setF, or the t = I variant behind surfG.g(), hits entries of its
 * predecessor.  Defaults: 512 grids and 8 GB in all, least recently used entries evicted first (one SCF cycle at a
 * fixed Fermi level is ~10^2 adaptive grids of 2 ... 324 points; BASELINE C3's 2000-point grid is 160 MB); 0 grids
 * switches the cache off and frees it (bench.py's headline runs cold that way).  Launches whose g would exceed 4 GB
 * are not cached.  The *_dev entry points download their energy list (16 bytes per point, one stream
 * synchronisation) to form the key while the cache is on.  Environment: NEGF_CHAIN_CACHE=<grids> presets max_grids. */
int negf_set_chain_cache(negf_ctx* ctx, int max_grids);
int negf_set_chain_cache_bytes(negf_ctx* ctx, long long max_bytes);
int negf_chain_cache_clear(negf_ctx* ctx);
/* counters since negf_create; entries / bytes currently held (any pointer may be NULL) */
int negf_chain_cache_stats(negf_ctx* ctx, long long* hits, long long* misses, long long* entries, long long* bytes);

/* ------------------------------------------------------ transmission eigenchannels
 * T(E) = sum_n T_n(E), T_n the eigenvalues of t^H t, t = Gamma_R^{1/2} G_RL Gamma_L^{1/2} (the reference has no such
 * function; it is the decomposition of its _transmission_kernel_restricted, transport.py:150-157).  For contacts L, R with
 * orbital lists I_L, I_R (|I_L| = K_L, |I_R| = K_R):
 *   Gamma_c = i (Sigma_c - Sigma_c^H) on I_c,  B = G[I_L,I_R] Gamma_R G[I_L,I_R]^H  (K_L x K_L, Hermitian PSD),
 *   Gamma_L = L L^H by PIVOTED Cholesky, truncated where the largest remaining diagonal is <= 1e-14 max diag Gamma_L
 *   (Gamma is PSD and often rank-deficient; L has r_L <= K_L columns),
 *   T_n = eigenvalues of H = L^H B L (r_L x r_L): the nonzero spectrum of t^H t.
 * When K_R < K_L the mirror form (L and R swapped, B = G[I_L,I_R]^H Gamma_L G[I_L,I_R]) puts the eigenproblem on the
 * smaller contact.  Output: nchan = min(K_L, K_R) values per energy in DESCENDING order, exact zeros beyond the
 * numerical rank, not clamped (a channel of -1e-17 is reported as such).  Sum rule: sum_n T_n = Re Tr[Gamma_L G
 * Gamma_R G^H], what negf_transmission returns, up to rounding and the truncation above.
 * Providers: those whose Gamma_c is confined to a known orbital list -- CONST when every contact's Sigma has a nonzero
 * support, CHAIN1D, BETHE without Xi; any other provider, the total self-energy as a contact, or min(K_L, K_R) > 96
 * return NEGF_EINVAL. */

/* ascending eigenvalues of m Hermitian K x K matrices (K <= 96), read from their lower triangles (imaginary parts of
 * the diagonal ignored) -- the reference's utils.eigh (utils.py:61-63) / numpy.linalg.eigvalsh, values only.  Parallel
 * cyclic complex Jacobi, one workgroup per matrix.  A_c128 [m][K][K], w [m][K]; info [m] or NULL: 0, 1 = non-finite
 * input (NaN row), 2 = not converged within the sweep limit; NEGF_ESINGULAR when any info is nonzero. */
int negf_eigvalsh_batched(negf_ctx* ctx, int K, int m, const double* A_c128, double* w, int* info);
/* min(K_L, K_R): the number of channels of (contact_L, contact_R); NEGF_EINVAL where the channels are not served */
int negf_channel_count(negf_ctx* ctx, int handle, int contact_L, int contact_R, int* nchan);
/* T_chan [m][nchan]: the min(nchan, count) largest channels, zeros in columns >= count.  info [m] or NULL as in
 * negf_transmission (a singular energy gives a NaN row, every one of its nchan columns); additionally -1 / -2 where the eigensolver met a non-finite
 * H / did not converge (NEGF_ESINGULAR then as well). */
int negf_transmission_channels(negf_ctx* ctx, int handle, int contact_L, int contact_R, int m, const double* E_c128,
                               int nchan, double* T_chan, int* info);
int negf_transmission_channels_dev(negf_ctx* ctx, int handle, int contact_L, int contact_R, int m, const double* E_dev,
                                   int nchan, double* T_chan_dev);

/* ------------------------------------------------------ eigenchannel scattering states
 * Which orbitals carry channel n (Paulsson and Brandbyge's eigenchannels; the reference has no such function).  For a
 * source contact s and a destination contact d with orbital lists I_s, I_d (K_s, K_d):
 *   Gamma_s = L L^H by the pivoted Cholesky above (rank r <= K_s),
 *   H = L^H G[I_d,I_s]^H Gamma_d G[I_d,I_s] L   (r x r, Hermitian PSD),   H u_n = T_n u_n, T_n descending,
 *   psi_n = G[:, I_s] L u_n   (an n-vector): the state injected from contact s by the retarded G in channel n,
 *   normalised to unit incoming flux.
 * The eigenproblem always lives on the SOURCE contact: nothing is divided by sqrt(T_n), closed channels have
 * well-defined states too.  To rounding: psi_a^H Gamma_d psi_b = T_a delta_ab (Gamma_d the n x n coupling of d);
 * sum_n T_n = negf_transmission(contact_L = d, contact_R = s); the nonzero T_n are those of
 * negf_transmission_channels(d, s); with all r channels sum_n psi_n psi_n^H = G Gamma_s G^H, the spectral function of
 * contact s (what negf_gless_int integrates).  Gauge: each psi_n carries the unit phase that makes its component of
 * largest |psi_i|^2 real and positive (lowest index on ties).  States inside a degenerate cluster of T_n are an
 * arbitrary orthogonal basis of that cluster.  All sums have a fixed order: results do not depend on negf_set_batch.
 * Providers as for negf_transmission_channels. */

/* numpy.linalg.eigh for m Hermitian K x K matrices (K <= 96), read from their lower triangles: w [m][K] ascending --
 * bitwise what negf_eigvalsh_batched returns, the same rotations --, V_c128 [m][K][K] with eigenvector j in column j
 * (the accumulated rotations, orthonormal to rounding).  info as in negf_eigvalsh_batched; a non-finite input gives
 * a NaN row of w and a NaN matrix V. */
int negf_eigh_batched(negf_ctx* ctx, int K, int m, const double* A_c128, double* w, double* V_c128, int* info);
/* K_s, the number of states contact_src injects; NEGF_EINVAL for providers the channels do not serve, for the total
 * self-energy as a contact and for K_s > 96 (K_d is not limited) */
int negf_channel_states_count(negf_ctx* ctx, int handle, int contact_src, int* count);
/* T_chan [m][nchan] descending and psi_c128 [m][nchan][n], each state contiguous.  Columns at or beyond the rank, or
 * at or beyond K_s, are exact zeros in both; a singular energy gives NaN rows in both and sets its info; info [m] or
 * NULL as in negf_transmission_channels (-1 / -2: the eigensolver met a non-finite H / did not converge).  The _dev
 * form keeps the grid and both results in HBM and is asynchronous. */
int negf_channel_states(negf_ctx* ctx, int handle, int contact_src, int contact_dst, int m, const double* E_c128,
                        int nchan, double* T_chan, double* psi_c128, int* info);
int negf_channel_states_dev(negf_ctx* ctx, int handle, int contact_src, int contact_dst, int m, const double* E_dev,
                            int nchan, double* T_chan_dev, double* psi_dev);

/* ------------------------------------------------------ local (bond) transmission
 * Where in the junction the current injected by contact `ind` flows (the reference has no such function; it is the
 * orbital-resolved form of its transmission, transport.py:150-157, built on the products of GrLessInt,
 * integrate.py:74-82).  Per energy, with K = E S - F (the assembled matrix WITHOUT the self-energies) and
 * A_c = G Gamma_c G^H, Gamma_c = i (Sigma_c - Sigma_c^H):
 *     flow[i][j] = 2 Im[K_ij A_c,ji]          -- transmission flowing from orbital i to orbital j.
 * For Hermitian F, S and real E it is real antisymmetric and conserves: for every split of the orbitals into
 * P (holding contact c's orbitals) and Q (holding every other contact's), sum_{i in P, j in Q} flow[i][j] is the total
 * transmission out of c -- Tr[Gamma_L G Gamma_R G^H] for two contacts --, and the row of an orbital outside all
 * contacts sums to zero.  Complex E and non-Hermitian F are not rejected: the formula is applied literally (the
 * conservation law then does not hold).  A_c,ji is read as conj(A_c,ij): providers whose coupling matrices were
 * handed in by the caller (negf_sigma_precomputed with gammas; they need not be Hermitian) return NEGF_EINVAL, and so
 * does n > 8192.  Every other provider negf_gless_int serves is served, ind as there.
 * group_of: host int[n], orbital -> group in [0, n_groups) (atoms, fragments, spin-resolved atoms; empty groups
 * allowed), or NULL with n_groups = n for every orbital its own group.  out [m][n_groups][n_groups]:
 *     out[k][a][b] = sum_{i in a, j in b} flow[i][j](E_k);
 * a singular energy gives a NaN table and its info, as negf_transmission.  All sums have a fixed order (no atomics):
 * results are bitwise equal from run to run, do not depend on negf_set_batch, and relabelling the groups permutes the
 * table bit for bit. */
int negf_local_transmission(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, int n_groups,
                            const int* group_of, double* out, int* info);
int negf_local_transmission_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, int n_groups,
                                const int* group_of, double* out_dev);
/* sum_k w_k flow(E_k) with REAL weights w [m], in one pass: out [n][n] float64.  Chunks of 32 consecutive energies of
 * the grid are added in order and the chunk sums in order, whatever the workspace batch.  A singular energy enters
 * as negf_gless_int's does (its info is set, NEGF_ESINGULAR returned). */
int negf_bond_int(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, const double* w,
                  double* out, int* info);
int negf_bond_int_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, const double* w_dev,
                      double* out_dev);

/* ------------------------------------------------------ overlap populations and projected DOS
 * Where the states sit and which contact fills them (the reference has no such function; its only density of states,
 * negf_dos = _dos_kernel, is -Im diag G / pi and ignores the overlap matrix: in a non-orthogonal basis that is not a
 * population).  Per energy, with G = (E S - F - sum_c Sigma_c)^-1, Gamma_c = i (Sigma_c - Sigma_c^H),
 * A_c = G Gamma_c G^H, and X = S (op = 0) or F (op = 1):
 *     ind = NEGF_IND_RETARDED:               pop[i][j]   = -(1/pi)  Im[G_ij   conj(X_ij)]
 *     ind = a contact / NEGF_IND_TOTAL
 *           (read as negf_gless_int does):   pop_c[i][j] = (1/2 pi) Re[A_c,ij conj(X_ij)]
 * conj(X_ij) is X_ji for the Hermitian F, S the quantities are defined for; otherwise the formula is applied literally.
 * X = S: the energy-resolved overlap population (COOP), whose row sums are the Mulliken-projected DOS
 * -Im (G S)_ii / pi and whose grand total is -Im Tr(G S) / pi; X = F: the Hamilton population (COHP).  For real E and
 * Hermitian F, S, i (G - G^H) = sum_c A_c exactly, hence  sum_c pop_c[i][j] = (pop[i][j] + pop[j][i]) / 2  (the two
 * sides come from different kernels and products).
 * group_of / n_groups as in negf_local_transmission (NULL with n_groups = n: every orbital its own group; empty groups
 * allowed).  rows_only = 0: out [m][n_groups][n_groups], out[k][a][b] = sum_{i in a, j in b} pop[i][j](E_k);
 * rows_only = 1: out [m][n_groups], out[k][a] = sum_b table[k][a][b] -- the projected DOS of atom / fragment a, in one
 * pass over G or A_c, the table never stored; each row is the sum of the very entries rows_only = 0 returns.
 * Providers: the retarded form serves every provider negf_dos serves; the contact form what negf_local_transmission
 * serves (coupling matrices handed in by the caller return NEGF_EINVAL: A_c need not be Hermitian then).  NEGF_EINVAL
 * also for op or rows_only outside {0, 1}, an invalid map and n > 8192.  A singular energy gives a NaN table / row and
 * its info, as negf_transmission.  All sums have a fixed order (no atomics): results are bitwise equal from run to run,
 * do not depend on negf_set_batch, and relabelling the groups permutes table and rows bit for bit.  The _dev form keeps
 * the grid and the result in HBM (group_of stays a host array) and is asynchronous. */
int negf_population(negf_ctx* ctx, int handle, int ind, int op, int rows_only, int m, const double* E_c128, int n_groups,
                    const int* group_of, double* out, int* info);
int negf_population_dev(negf_ctx* ctx, int handle, int ind, int op, int rows_only, int m, const double* E_dev,
                        int n_groups, const int* group_of, double* out_dev);
/* Projection on k vectors w_a (W_c128 [k][n], each vector contiguous, 1 <= k <= n; fragment orbitals: pass w = S c for
 * orbital coefficients c, <phi|G|phi> = c^H S G S c in a non-orthogonal basis):
 *     ind = NEGF_IND_RETARDED:  p_a   = -(1/pi)  Im[w_a^H G   w_a]
 *     contact form:             p_c,a = (1/2 pi) Re[w_a^H A_c w_a]
 * out [m][k].  One batched product Y = G W^T (or A_c W^T) with W shared by the batch, then w_a^H y_a column by column.
 * For real E and Hermitian F, S: sum_c p_c,a = p_a; for a complete S-orthonormal set C (C^H S C = 1, w = S c):
 * sum_a p_a = -Im Tr(G S) / pi, the sum of negf_population's rows with X = S.  Providers, NaN / info and NEGF_EINVAL as
 * for negf_population; k outside 1 .. n is NEGF_EINVAL.  Every sum has a fixed order that depends on n alone: bitwise
 * equal from run to run, independent of negf_set_batch, and p_a does not depend on k or on the other vectors.  In the
 * _dev form the grid, W and the result are in HBM. */
int negf_projected_dos(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, int k, const double* W_c128,
                       double* out, int* info);
int negf_projected_dos_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, int k, const double* W_dev,
                           double* out_dev);

/* --------------------------------------------- multi-terminal transmission matrix and probes
 * All transmissions between the terminals of a junction from ONE inverse per energy (negf_transmission serves one pair
 * per call and inverts again for the next; the reference has no such function, and lists decoherence under "Future
 * development" of its constant self-energy provider).  Terminals: the provider's contacts 0 .. n_c - 1, followed by
 * n_probes probes, C = n_c + n_probes.  Probe p is an orbital list I_p (probe_nk[p] distinct indices in [0, n),
 * concatenated in probe_inds) and a K_p x K_p complex block Sigma_p (concatenated in probe_sigma_c128, row-major): a
 * fictitious, energy-independent contact (Buettiker / D'Amato-Pastawski).  The block need not be anti-Hermitian;
 * probes may overlap each other and the leads.  Per energy
 *     A(E)   = E S - F - Sigma_provider(E) - sum_p scatter(Sigma_p on I_p x I_p),    G = A^-1
 *     Gamma_a = i (Sigma_a - Sigma_a^H)      on terminal a's orbital list (a contact's block, or a probe's)
 *     T[a][b] = Re Tr[Gamma_a G Gamma_b G^H] = Re sum_{i in I_a, j in I_b} (Gamma_a G_ab Gamma_b)_ij conj(G_ab,ij),
 *     G_ab = G[I_a, I_b]
 * T [m][C][C].  T[a][b] is the transmission from b into a: T[L][R] is what negf_transmission(L, R) returns.  The
 * diagonal is the same formula with a = b (not a reflection).  For real E, Hermitian F, S and Gamma >= 0: T[a][b] >= 0,
 * the sums of row a and of column a agree (current conservation), T = T^T for real-symmetric F, S, Sigma and in general
 * NOT for complex-Hermitian F.  n_probes = 0 (the pointers may be NULL): the matrix over the contacts alone.
 * Providers: those whose Gamma_c lives on a known orbital list, as for negf_transmission_channels -- CONST with a
 * nonzero support per contact, CHAIN1D (both solvers; the g(E) cache behaves as in any other call), BETHE without Xi;
 * the lists may cover any share of the orbitals.  NEGF_EINVAL: any other provider, an invalid probe list (size outside
 * 1 .. n, an index outside [0, n) or named twice in one probe), C > 1024.  The total self-energy is not a terminal.
 * A singular energy gives a NaN matrix and its info, as negf_transmission; the other energies are unaffected.
 * Work per energy: K_tot sum_a K_a^2 complex multiply-adds (K_tot = sum_a K_a) behind the one inverse.  No atomics,
 * every sum in an order fixed by the pair's own (K_a, K_b): results are bitwise equal from run to run, do not depend on
 * negf_set_batch, and permuting the probes permutes rows and columns of T bit for bit.  The _dev form keeps the grid
 * and the result in HBM (the probe arrays stay host arrays) and is asynchronous; info via negf_last_info.
 * Profile family: "tmat". */
int negf_transmission_matrix(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                             const double* probe_sigma_c128, int m, const double* E_c128, double* T, int* info);
int negf_transmission_matrix_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                 const double* probe_sigma_c128, int m, const double* E_dev, double* T_dev);

/* --------------------------------------------- floating dephasing probes: response, G^<, G^r
 * The probes of negf_transmission_matrix (same arguments, same providers, same NEGF_EINVAL cases) left FLOATING: at every
 * energy each probe takes the occupation at which it draws no net current.  Per energy, with T the transmission matrix
 * over the C = n_c + n_probes terminals and To = T with zero diagonal,
 *     W_pp = sum_{c != p} To[p][c] (c over ALL terminals),   W_pq = -To[p][q],   P' = the probes with W_pp > 0,
 *     R[P', :] = W^-1 To[P', 0 .. n_c)        rows of probes outside P' (decoupled probes) are exact zeros
 * R [m][n_probes][n_c] is the probes' response to the real contacts: probe p's occupation is f_p(E) = sum_c R[p][c] f_c(E).
 * W is a weakly row-diagonally-dominant M-matrix and W 1 = To[P', real] 1: for real E, Hermitian F, S and Gamma >= 0
 * every row of R over P' sums to 1 and 0 <= R <= 1 to rounding.  The floating condition is a real-axis notion; complex
 * energies are not rejected and the formulas are applied literally (as negf_local_transmission applies its own).
 * The solve is LU without pivoting (backward stable for such W; dominance survives elimination), one workgroup per
 * energy, rows and columns in an order derived from the probes' content: results are bitwise equal from run to run, do
 * not depend on negf_set_batch, and permuting the probes permutes the rows of R bit for bit.  An energy that is singular,
 * or whose T holds a non-finite entry, gives a NaN R and its info, as negf_transmission_matrix.  Probes that reach no
 * contact at an energy (a cluster that sees only itself) make W singular and leave the occupations undefined: the
 * elimination meets a pivot that is not positive and the WHOLE R of that energy is NaN, info stays 0 (the inverse was
 * regular); negf_gless_int_probes' sum for a contact is then NaN as well.  The test is on the pivot as computed: a cluster
 * whose path to the contacts is merely tiny gives an ill-conditioned W and an R as inaccurate as that.  n_probes = 0: nothing
 * is written (R may be NULL).  The _dev form keeps the grid and the result in HBM and is asynchronous.
 * Profile families: "tmat" (the matrices), "deph" (the solve and the coupling assembly below). */
int negf_probe_response(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                        const double* probe_sigma_c128, int m, const double* E_c128, double* R, int* info);
int negf_probe_response_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                            const double* probe_sigma_c128, int m, const double* E_dev, double* R_dev);
/* The lesser Green's function's weighted sum with floating probes, G^< = i sum_c f_c G D_c G^H:
 *     out = sum_k w_k G(E_k) D_s(E_k) G(E_k)^H,    D_s = scatter(Gamma_s on I_s) + sum_p R[p][s] scatter(Gamma_p on I_p)
 * with G = A^-1 of the A that carries the probes (negf_transmission_matrix) -- one inverse per energy, the response and
 * the coupling assembled on the device.  `ind` is read as negf_gless_int reads it; NEGF_IND_TOTAL: D = the sum of ALL
 * terminals' Gamma (no solve).  The D_s of the contacts add up to that total, Re Tr[Gamma_d G D_s G^H] (d != s) is the
 * effective transmission with the probes floating, and probes of zero strength give negf_gless_int's result.  The
 * contacts' matrices are the blocks negf_transmission_matrix uses.  out is n x n, Hermitian for real weights.  A singular
 * energy enters as negf_gless_int's does.  Overlapping probes are added in an order derived from their content: the
 * result does not depend on the caller's probe order, nor on negf_set_batch: the weighted sum adds the energies
 * [32 c, 32 c + 32) OF THE GRID from zero, then the chunk sums in ascending order, and a chunk that a sweep boundary cuts
 * waits in a carry buffer for the next sweep (negf_bond_int's order). */
int negf_gless_int_probes(negf_ctx* ctx, int handle, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                          const double* probe_sigma_c128, int m, const double* E_c128, const double* w_c128,
                          double* out_c128, int* info);
int negf_gless_int_probes_dev(negf_ctx* ctx, int handle, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                              const double* probe_sigma_c128, int m, const double* E_dev, const double* w_dev,
                              double* out_dev);
/* sum_k w_k G(E_k) with the probes in A: negf_gr_int's pass on the matrix that carries them.  The probes do not depend
 * on the energy, so the contour integrals stay valid. */
int negf_gr_int_probes(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                       const double* probe_sigma_c128, int m, const double* E_c128, const double* w_c128,
                       double* out_c128, int* info);
int negf_gr_int_probes_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                           const double* probe_sigma_c128, int m, const double* E_dev, const double* w_dev,
                           double* out_dev);

/* --------------------------------------------- layered devices: the recursive Green's function
 * Wires, oligomers between chain leads, molecules with several principal layers of electrode: systems whose orbitals
 * fall into L >= 2 layers that couple to their neighbours only.  Every entry point above inverts the full N x N matrix
 * E S - F - Sigma(E) per energy (8 N^3 flops, 16 N^2 bytes); these do L inverses and a handful of products of LAYER size
 * per energy (the recursive Green's function; the reference has no such path -- each call names the reference function
 * whose dense form it replaces).
 * A layered system is an object of its own inside the context, with its own handle, terminals and workspace; nothing
 * here reads or changes the dense system of negf_set_system, its providers or their results.
 *   blocks   F_ii, S_ii (n_i x n_i) and the upper couplings F_{i,i+1}, S_{i,i+1} (n_i x n_{i+1}), row-major, concatenated
 *            in layer order; the lower blocks are their conjugate transposes (F, S Hermitian, real or complex); the
 *            sizes n_i are arbitrary, 1 .. 8192 each.
 *   per energy, A_ij = E S_ij - F_ij:
 *            g_0 = (A_00 - Sigma_left)^-1,  g_i = (A_ii - A_{i,i-1} g_{i-1} A_{i-1,i} - [i = L-1] Sigma_right)^-1
 *            X_0 = g_0, X_i = -g_i A_{i,i-1} X_{i-1} = G_{i,0};   Y_i = -Y_{i-1} A_{i-1,i} g_i = G_{0,i}
 *            G_{L-1,L-1} = g_{L-1},  G_ii = g_i + g_i A_{i,i+1} G_{i+1,i+1} A_{i+1,i} g_i,
 *            G_{i,i+1} = -g_i A_{i,i+1} G_{i+1,i+1},  G_{i+1,i} = -G_{i+1,i+1} A_{i+1,i} g_i
 * NEGF_EINVAL before anything is launched: fewer than two layers, a layer size outside 1 .. 8192, an index list that
 * leaves its layer or names an orbital twice, a terminal on an interior layer, more than 8 terminals on one end, a
 * transmission between terminals of the same end, more energies than a `blocks` terminal was given.
 * A singular layer sets info[k] = the 1-based column of the zero pivot counted over the whole system and returns
 * NEGF_ESINGULAR, as the dense calls do.  negf_set_batch and negf_set_inverse_algo apply.  Every sum has a fixed order:
 * results are bitwise equal from run to run, do not depend on negf_set_batch, and permuting the energies permutes them.
 * Not served: eigenchannels, flows with floating probes,
 * TERMINALS (leads) on interior layers -- probes, which are arguments of negf_layered_transmission_matrix, may sit on any
 * layer --, spin layouts other than 'r', sharding, checkpoints. */
int negf_layered_create(negf_ctx* ctx, int n_layers, const int* sizes, const double* F_diag_c128, const double* F_up_c128,
                        const double* S_diag_c128, const double* S_up_c128, int* handle);
int negf_layered_free(negf_ctx* ctx, int handle);
/* Terminals: a self-energy block Sigma_t on K distinct orbitals `inds` (counted inside the layer) of layer 0 or layer
 * L - 1; several may share an end layer and orbitals (they are subtracted in the order they were made).  *terminal
 * numbers them from 0.
 *   const:  one K x K block for all energies -- surfGTester.py:94-132 restricted to its support.
 *   chain:  the 1-D chain lead of negf_sigma_chain1d (surfG1D.py:223-399) with one contact; solver 0 = the reference's
 *           relaxed fixed point (conv, relFactor, max_iter), 1 = renormalisation-decimation (conv = tol, max_iter =
 *           max_steps, force_iters = force_steps; negf_sigma_chain1d_rd).  It runs through the same kernels and the same
 *           g(E) cache: its Sigma is bitwise what negf_sigma_eval gives for that lead and energy on a dense system.
 *   blocks: [m][K][K] blocks supplied per energy (Bethe lattices, foreign self-energies: negf_sigma_precomputed's role,
 *           integrate.py:169,203-204); block k serves energy k of every later call. */
int negf_layered_terminal_const(negf_ctx* ctx, int handle, int layer, int K, const int* inds, const double* sigma_c128,
                                int* terminal);
int negf_layered_terminal_chain(negf_ctx* ctx, int handle, int layer, int K, const int* inds,
                                const double* alpha, const double* Salpha, const double* beta, const double* Sbeta,
                                const double* tau, const double* Stau, double eta, double conv, double relFactor,
                                int max_iter, int force_iters, int solver, int* terminal);
int negf_layered_terminal_blocks(negf_ctx* ctx, int handle, int layer, int K, const int* inds, int m,
                                 const double* sigma_c128, int* terminal);
/* Sigma_t(E) itself, [m][K][K] -- g.sigma(E, i) on the terminal's orbitals (surfG1D.py:344-399) */
int negf_layered_terminal_sigma(negf_ctx* ctx, int handle, int terminal, int m, const double* E_c128,
                                double* sigma_out_c128);
/* T_ab(E) = Re Tr[Gamma_a G_ab Gamma_b G_ab^H], G_ab = G[I_a, I_b] cut from the corner block G_{L-1,0} (a on the last
 * layer) or G_{0,L-1} (a on layer 0) -- _transmission_kernel_restricted, transport.py:150-157; T [m].  T_ab is the
 * transmission from b into a, what negf_transmission(L = a, R = b) returns on the dense system; G is not symmetric for
 * complex F, so T_ab != T_ba in general.  One forward sweep, no g_i kept: 10 matrices of the largest layer per energy in
 * flight, whatever L. */
int negf_layered_transmission(negf_ctx* ctx, int handle, int term_a, int term_b, int m, const double* E_c128,
                              double* T, int* info);
int negf_layered_transmission_dev(negf_ctx* ctx, int handle, int term_a, int term_b, int m, const double* E_dev,
                                  double* T_dev);
/* form 0: -Im diag G / pi -- _dos_kernel, transport.py:183-190; form 1: the Mulliken form -Im diag(G S) / pi, which
 * reads the blocks G_{i,i+-1} as well (the rows of negf_population's overlap table).  dos_total [m], dos_site [m][N]
 * (N = sum n_i, orbitals in layer order; may be NULL in the host form only). */
int negf_layered_dos(negf_ctx* ctx, int handle, int form, int m, const double* E_c128, double* dos_total,
                     double* dos_site, int* info);
int negf_layered_dos_dev(negf_ctx* ctx, int handle, int form, int m, const double* E_dev, double* dos_total_dev,
                         double* dos_site_dev);
/* sum_m w_m G(E_m) on the pattern of S -- GrInt, integrate.py:146-173.  out = the diagonal blocks G_ii, then the upper
 * blocks G_{i,i+1}, then the lower blocks G_{i+1,i} (n_{i+1} x n_i), each row-major, concatenated in layer order:
 * sum n_i^2 + 2 sum n_i n_{i+1} complex values.  Energy k enters every element's sum after energy k - 1. */
int negf_layered_gr_int(negf_ctx* ctx, int handle, int m, const double* E_c128, const double* w_c128,
                        double* out_c128, int* info);
int negf_layered_gr_int_dev(negf_ctx* ctx, int handle, int m, const double* E_dev, const double* w_dev,
                            double* out_dev);
/* A_c = G Gamma_c G^H on the pattern of S, Gamma_c = i (Sigma_c - Sigma_c^H).  A terminal touches K orbitals J of its end
 * layer, so only the columns W_i = G_{i,end}[:, J] (n_i x K) are formed, from what the two sweeps hold anyway:
 *   terminal on the last layer:  W_{L-1} = G_{L-1,L-1}[:, J],  W_i = g_i C_{i,i+1} W_{i+1}                  (C = -A)
 *   terminal on layer 0:         x_0 = g_0[:, J],  z_i = C_{i,i-1} x_{i-1},  x_i = g_i z_i  (forward, the z_i kept);
 *                                W_0 = G_00[:, J],  W_i = G_ii z_i                          (backward)
 *   A_ii = (W_i Gamma) W_i^H,  A_{i,i+1} = (W_i Gamma) W_{i+1}^H;  A_{i+1,i} = A_{i,i+1}^H is never formed.
 * `ind`: a terminal number in [-n_t, n_t), negative values counted from the end as negf_gless_int reads them, or
 * NEGF_IND_TOTAL = all terminals of both ends.  Each end has ONE column set on the union of the selected terminals'
 * orbitals (ascending); its Gamma is the sum of theirs in the order the terminals were made, and the contribution of
 * layer 0's set to an element is added before the last layer's.  NEGF_EINVAL before anything is launched: an unknown
 * handle, `ind` outside the range, NEGF_IND_TOTAL on a system without terminals, more energies than a `blocks` terminal
 * holds, null pointers.  A singular layer reports as negf_layered_gr_int's does.
 *
 * negf_layered_gless_int: sum_k w_k A(E_k) -- GrLessInt, integrate.py:177-208 (densityGrid, density.py:605-658), in
 * negf_layered_gr_int's layout.  The weights are complex: the lower blocks are sum_k w_k conj(A_{i,i+1}(E_k))^T, which is
 * the conjugate transpose of the upper sum only for real weights.  Energy k enters every element's sum after k - 1. */
int negf_layered_gless_int(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, const double* w_c128,
                           double* out_c128, int* info);
int negf_layered_gless_int_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, const double* w_dev,
                               double* out_dev);
/* The contact-resolved Mulliken PDOS, dos_site[k][i] = (1/2pi) Re sum_j A_ij(E_k) conj(S_ij) over the pattern -- the rows
 * of negf_population's contact form with X = S, rows_only = 1 (calculate_pdos with a contact); dos_total[k] = their sum.
 * dos_total [m], dos_site [m][N] (may be NULL in the host form only). */
int negf_layered_contact_dos(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, double* dos_total,
                             double* dos_site, int* info);
int negf_layered_contact_dos_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, double* dos_total_dev,
                                 double* dos_site_dev);
/* The transmission matrix T[k][a][b] = Re Tr[Gamma_a G Gamma_b G^H](E_k) between ALL terminals -- negf_transmission_matrix's
 * definition and orientation (the transmission from b into a) on a layered system; T [m][C][C].  The terminals are the
 * system's end terminals in the order they were made, then the call's n_probes probes, C = n_t + n_probes.  Probe p is
 * probe_nk[p] distinct orbitals (probe_inds, concatenated; numbered in the WHOLE system in layer order) that all lie in
 * ONE layer -- any layer -- and an energy-independent probe_nk[p] x probe_nk[p] block Sigma_p (probe_sigma, concatenated),
 * subtracted from A_ll beside the terminals' blocks; probes may overlap each other and the leads, and overlapping probes
 * enter A in an order derived from their content (size, orbital list, values), not from the caller's order.
 * With J_q = the ascending union of the orbitals of the terminals on layer q and K_tot = sum |J_q|, a backward sweep carries
 *   strip_{L-1} = [G_{L-1,L-1}[:, J_{L-1}]],   strip_i = [G_ii[:, J_i] | g_i C_{i,i+1} strip_{i+1}]      (n_i x sum_{q>=i} |J_q|)
 * which holds G_{i,q}[:, J_q] for every q >= i: the pairs (a on layer i, b on a layer >= i) are read from it and the strip
 * is dropped; the pairs with b on an earlier layer come from the same pass over the layers in reverse order.  No block
 * G_iq of two distant layers is ever formed: O(L n^3 + L n^2 K_tot) flops and O(L n^2 + n K_tot) memory per energy.
 * n_probes = 0 gives the matrix over the end terminals, pairs on the SAME end included.
 * NEGF_EINVAL before anything is launched: an unknown handle, a probe that leaves [0, N), names an orbital twice or spans
 * two layers, C > 1024, C = 0, more energies than a `blocks` terminal holds.  A singular layer gives a NaN matrix for
 * that energy, its info (the whole-system column) and NEGF_ESINGULAR; other energies are unaffected.  No floating-point
 * atomics; results are bitwise equal from run to run, independent of negf_set_batch, and permuting the probes permutes
 * rows and columns of T bit for bit. */
int negf_layered_transmission_matrix(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                     const double* probe_sigma_c128, int m, const double* E_c128, double* T, int* info);
int negf_layered_transmission_matrix_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk,
                                         const int* probe_inds, const double* probe_sigma_c128, int m, const double* E_dev,
                                         double* T_dev);
/* The probes of negf_layered_transmission_matrix left FLOATING at every energy -- negf_probe_response,
 * negf_gless_int_probes and negf_gr_int_probes on a layered system, results on the pattern of S.  Terminals and probe
 * arguments are negf_layered_transmission_matrix's, with the same NEGF_EINVAL cases before anything is launched; `ind` is
 * read as negf_layered_gless_int reads it.
 * negf_layered_probe_response: R [m][n_probes][n_t], probe p's occupation at E_k is sum_c R[k][p][c] f_c(E_k).  With To = T
 * with zero diagonal: W_pp = sum_{c != p} To[p][c] over ALL terminals, W_pq = -To[p][q], P' = the probes with W_pp > 0,
 * R[P', :] = W^-1 To[P', 0:n_t], exact zeros outside P' (negf_probe_response's rules with n_c -> n_t).  NaN R: a pivot
 * that is not positive (probes that reach no end terminal) makes the whole energy NaN with info 0; a singular layer gives
 * its info and NEGF_ESINGULAR.  With n_probes = 0 nothing is written.
 * negf_layered_gless_int_probes: sum_k w_k A(E_k), A = G D_s G^H with D_s = scatter(Gamma_s) + sum_p R_ps scatter(Gamma_p)
 * (ind = NEGF_IND_TOTAL: the sum of all terminals' Gamma, no solve) and G the inverse of the matrix that carries the
 * probes, in negf_layered_gr_int's block layout with complex weights: diagonal blocks, upper blocks A_{i,i+1}, lower blocks
 * sum_k w_k conj(A_{i,i+1}(E_k))^T.  Every terminal lives in one layer, so D = (+)_q D_q is block diagonal on the union
 * lists J_q.  R needs the whole T before D exists: the two strip passes KEEP the strips of all layers, Cfull_i = [G_{i,q}[:,
 * J_q]]_q (n_i x K_tot; the blocks q >= i from the pass over the layers as they are, the others from the reversed pass),
 * then Y_i = Cfull_i blockdiag(D_q) for all layers in one launch, A_ii = Y_i Cfull_i^H, A_{i,i+1} = Y_i Cfull_{i+1}^H: one
 * inverse per layer, pass and energy, nothing recomputed.  Energy k enters every element's sum after k - 1.
 * negf_layered_gr_int_probes: sum_k w_k G(E_k) on the pattern with the probes in A, negf_layered_gr_int's layout.
 * The _dev forms follow the stream contract of the device-resident variants: they overwrite out_dev / R_dev, and the
 * host tables of the probes are uploaded with a wait.  No floating-point atomics; results are bitwise equal from run to
 * run, independent of negf_set_batch, permuting the probes permutes the rows of R bit for bit and leaves the sums bit
 * for bit, permuting the energies permutes R.  Profile family of the two new kernels: "deph". */
int negf_layered_probe_response(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                const double* probe_sigma_c128, int m, const double* E_c128, double* R, int* info);
int negf_layered_probe_response_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                    const double* probe_sigma_c128, int m, const double* E_dev, double* R_dev);
int negf_layered_gless_int_probes(negf_ctx* ctx, int handle, int ind, int n_probes, const int* probe_nk,
                                  const int* probe_inds, const double* probe_sigma_c128, int m, const double* E_c128,
                                  const double* w_c128, double* out_c128, int* info);
int negf_layered_gless_int_probes_dev(negf_ctx* ctx, int handle, int ind, int n_probes, const int* probe_nk,
                                      const int* probe_inds, const double* probe_sigma_c128, int m, const double* E_dev,
                                      const double* w_dev, double* out_dev);
int negf_layered_gr_int_probes(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                               const double* probe_sigma_c128, int m, const double* E_c128, const double* w_c128,
                               double* out_c128, int* info);
int negf_layered_gr_int_probes_dev(negf_ctx* ctx, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                   const double* probe_sigma_c128, int m, const double* E_dev, const double* w_dev,
                                   double* out_dev);
/* Where the current injected by the terminals `ind` flows -- negf_local_transmission / negf_bond_int on a layered system:
 *   flow[i][j](E) = 2 Im[K_ij A_ji],  K = E S - F,  A = G Gamma G^H of negf_layered_gless_int for the same `ind`.
 * K is zero wherever S and F are, so the complete orbital-resolved flow lives on the pattern of S, nothing truncated:
 *   diagonal block i:     flow[r][c] = 2 Im[K_ii[r][c] conj(A_ii[r][c])]
 *   upper block (i, i+1): flow[r][c] = 2 Im[K_u[r][c] conj(A_u[r][c])]
 *   lower block (i+1, i): flow[r][c] = 2 Im[K_l[r][c] A_u[c][r]]        (a transposed read of the upper block of A)
 * (A_ii = (W Gamma) W^H is Hermitian to the rounding of its products only: the diagonal block's flow reads its Hermitian part
 * (A_ii + A_ii^H) / 2, so that at real E every block of the flow is antisymmetric bit for bit, flow_l = -flow_u^T included)
 * applied literally for complex E as well (then the flow is not conserved and the lower block is not minus the
 * transpose of the upper one).  K is formed per element from E and the stored blocks of S and F and never stored.  For
 * one injecting terminal at real E the sum of upper block i -- the flow from layer i into layer i + 1 -- is the
 * transmission, at every one of the L - 1 boundaries.
 * negf_layered_local_transmission: per energy.  groups_per_layer (host int[L], g_i >= 1) and group_of (host int[N]: for
 * each orbital in layer order its group inside its own layer, in [0, g_i); empty groups are allowed) reduce each block
 * to out[a][b] = sum_{r in a, c in b} flow[r][c]; both NULL: every orbital its own group (g_i = n_i).  out: doubles in
 * negf_layered_gr_int's block order with g in place of n -- diagonal g_i x g_i, upper g_i x g_{i+1}, lower g_{i+1} x g_i --
 * and [m] of those.  The order of the additions depends on the orbitals' positions inside their groups only: relabelling
 * the groups permutes the tables bit for bit.  A singular layer gives a NaN table for that energy, its info (the
 * whole-system column) and NEGF_ESINGULAR; other energies are unaffected.
 * negf_layered_bond_int: sum_k w_k flow(E_k) with REAL weights w [m] (doubles) at orbital level, sum n_i^2 +
 * 2 sum n_i n_{i+1} doubles in the same order; energy k enters every element's sum after k - 1, and a singular energy
 * enters it as it enters negf_layered_gless_int's.
 * NEGF_EINVAL before anything is launched: an unknown handle, `ind` as negf_layered_gless_int refuses it, a group_of entry
 * outside its layer's range, exactly one of the two group pointers NULL, g_i < 1, more energies than a `blocks` terminal
 * holds, null pointers.  No floating-point atomics; results are bitwise equal from run to run, independent of
 * negf_set_batch, and permuting the energies permutes the per-energy tables.  Profile family "bond". */
int negf_layered_local_transmission(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128,
                                    const int* groups_per_layer, const int* group_of, double* out, int* info);
int negf_layered_local_transmission_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev,
                                        const int* groups_per_layer, const int* group_of, double* out_dev);
int negf_layered_bond_int(negf_ctx* ctx, int handle, int ind, int m, const double* E_c128, const double* w, double* out,
                          int* info);
int negf_layered_bond_int_dev(negf_ctx* ctx, int handle, int ind, int m, const double* E_dev, const double* w_dev,
                              double* out_dev);
/* device bytes of the work areas of the system's last call: (10 + L for a backward sweep) matrices of the largest layer
 * per energy in flight, and for a G Gamma G^H call its column sets -- with cs = n_max K_max: (L + 4) cs + K^2 for the set of
 * layer 0 (the z_i, x twice, W twice, Y, Gamma), 3 cs + K^2 for the last layer's.  For a transmission-matrix call, per
 * energy in flight: the 10 + L matrices, two strips of n_max K_tot, the Gamma blocks of the chain and blocks terminals and
 * three K_a K_b areas of the largest pair that takes the matrix-core path; once per call: the Gamma blocks of the probes
 * and const terminals (sum K^2).  The result [m][C][C] is the caller's.  A bond call (negf_layered_local_transmission,
 * negf_layered_bond_int) is a G Gamma G^H call plus, with groups, the maps (N + sum (g_i + 1) ints) and, in the host form,
 * the staging of its result (m tables / one table of doubles).  The floating-probe calls: negf_layered_probe_response is
 * a transmission-matrix call plus C^2 doubles per energy in flight (the matrices of the batch); negf_layered_gr_int_probes
 * the 10 + L matrices and the once-per-call Gamma blocks; negf_layered_gless_int_probes, per energy in flight, the 10 + L
 * matrices, the KEPT strips and Y of all layers (2 L n_max K_tot elements, in place of the two alternating strips), the
 * Gamma blocks that depend on E, the three K_a K_b areas, D (sum_q |J_q|^2 elements) and -- for a contact with probes --
 * C^2 + n_probes n_t doubles (T and R); once per call the Gamma blocks of the probes and const terminals. */
int negf_layered_workspace_bytes(negf_ctx* ctx, int handle, long long* work);

/* ------------------------------------------------------------- diagnostics */
/* hipEvent timing of the library's own kernels, per kernel family
 * ("inverse", "assemble", "accumulate", "zgemm", "trace", "chain1d", "bethe", "eig", "bond", "pop", "tmat", "deph";
 * "chain1d_rd": the renormalisation-decimation solver's launches, "chain1d_hit" / "chain1d_rd_hit": g(E) cache hits). */
/* device bytes held by the context's energy workspace: the three n x n work areas per energy in flight (work) and the
 * staging of the self-energy blocks of CHAIN1D / BETHE providers (blocks); either pointer may be NULL */
int negf_workspace_bytes(negf_ctx* ctx, long long* work, long long* blocks);
int negf_profile_enable(negf_ctx* ctx, int on);
int negf_profile_reset(negf_ctx* ctx);
int negf_profile_read(negf_ctx* ctx, const char* family, double* total_ms, int* launches);
/* flops of the family's launches since negf_profile_reset, two ways: ALGORITHMIC (8 per complex multiply-add: 8 M N K
 * per dense product, 8 n^3 per inverse -- what the reference's solve / matmul would be charged) and ISSUED
 * to the matrix cores (the kernels use the 3-real-product form of a complex product, compute 16-granular tiles, skip
 * the lower block tiles of Hermitian products; pivot steps and other vector work are not matrix-core flops).  Only
 * the second may be divided by the FP64 MFMA peak and called utilisation.  Families: "inverse", "zgemm". */
int negf_profile_read_flops(negf_ctx* ctx, const char* family, double* flops_algorithmic, double* flops_mfma_issued);
/* choose the inverse kernel: 0 = auto, 1 = unblocked Gauss-Jordan (any n),
 * 2 = blocked Gauss-Jordan with FP64 MFMA trailing updates (window kernel by size and batch),
 * 3 = the same with the register-strip window kernel wherever it exists (64 <= n <= 1024; tests, A/B),
 * 4 = the same with the team window kernels / the single-workgroup kernel only (the round-4 configuration) */
int negf_set_inverse_algo(negf_ctx* ctx, int algo);
/* systems of n <= 96 orbitals: 0 = auto -- with negf_set_inverse_algo(0), E S - F - Sigma is assembled, inverted and
 * (GrInt) accumulated in ONE kernel with the matrix held in the registers of a compute unit (no n x n work area in
 * HBM; the SCF call pattern is ~10^2 integrals of 2 ... 324 points per density step, scfE.py:301-462); 1 = the
 * assemble / inverse / accumulate kernel sequence through HBM that larger systems use (cross-check, A/B) */
int negf_set_small_algo(negf_ctx* ctx, int algo);
/* CHAIN1D launches with more fixed points (energy x contact) than the device holds at once: the fixed points differ
 * up to 20x in their sweep counts (surfG1D.py:271-288 stops each at its own residual), and the counts are unknown
 * before the first evaluation.  The kernel runs them ROUND ROBIN: one persistent workgroup per resident slot, a fixed
 * point runs `quantum` sweeps and, when others wait, goes to the back of a device-side queue with its iterate.  The
 * chip then stays full until fewer fixed points than slots are left, whatever order they were started in; results
 * do not depend on it (a fixed point is a sequence of sweeps on its own data).  quantum: < 0 = default -- quanta of
 * 100 sweeps for every such launch, whether or not its sweep counts can be predicted from the
 * provider's previous evaluation (on the C3 grid the queue is 1.5 % faster than one workgroup per fixed point started
 * longest first, and its initial order is worth nothing); 0 = never round robin: one workgroup per fixed point, longest
 * first by the predicted counts; > 0 = this quantum.  Launches that fit the device, or whose sweep cap is not above
 * the quantum, always run one workgroup per fixed point.  slots: 0 = every resident slot of the device; > 0 caps them
 * (tests). */
int negf_set_chain_round_robin(negf_ctx* ctx, int quantum, int slots);
/* G Gamma G^H (integrate.py:81) and Tr[Gamma_L G Gamma_R G^H] (transport.py:156-157):
 * 0 = auto -- when the coupling matrices only touch the contact orbitals (CONST providers
 * with a small support, CHAIN1D / BETHE blocks without an orthogonalisation matrix) the
 * products run on the columns / the block of G on those orbitals only (same sums, the
 * terms that are exactly zero are skipped); 1 = always the dense n x n products */
int negf_set_gamma_algo(negf_ctx* ctx, int algo);
/* run the FP64 MFMA fragment-layout probe; max abs error vs an exact integer
 * product (0.0 expected) */
int negf_selftest_mfma(negf_ctx* ctx, double* max_err);
/* The batched complex product kernels behind every G Gamma G^H, transmission and channel product, called directly on
 * operands of the caller's choice (a diagnostic call for tests: every call allocates, uploads and downloads):
 *     C_b = A_b op(B_b),  b < nb,   A_b M x K (row-major, leading dimension lda >= K),
 * opB bit 0: op(B) = B^H with B stored N x K (ldb >= K), else B is K x N (ldb >= N); bit 1: the caller promises a
 * Hermitian product (M == N): the block tiles on and above the diagonal are computed, those above it mirrored; bit 2:
 * the result is stored conjugate-transposed, N x M (ldc >= M; else M x N, ldc >= N).  Bit 1 is dropped where M != N
 * or bit 2 is set.  Strides are in complex elements; strideA / strideB = 0 shares the operand among the batch,
 * otherwise a stride is at least rows * ld, and so is strideC always.  The host arrays hold nb * stride complex values
 * (rows * ld for a shared operand).  ALL of C is uploaded before the launch and downloaded after it, so the caller
 * sees which elements the kernel wrote.  kernel: 0 = the production rule (negf_zgemm_plan), 1 = the 64 x 64 block
 * kernel, 2 = the flexible-block kernel, 3 = the vector-unit kernel (four-product form, ignores bit 1).  K = 0 gives
 * zeros.  NEGF_EINVAL: a null pointer, M or N < 1, K < 0, nb < 1, opB outside 0 .. 7, kernel outside 0 .. 3, a
 * leading dimension or stride below the above, an array of more than 2^31 elements. */
int negf_zgemm_batched(negf_ctx* ctx, int M, int N, int K, int nb, const double* A_c128, int lda, long long strideA,
                       const double* B_c128, int ldb, long long strideB, int opB, double* C_c128, int ldc,
                       long long strideC, int kernel);
/* What negf_zgemm_batched does with a shape; a host function that needs no device.  kernel as above (0: the rule the
 * library's own products follow -- the flexible kernel where the 64 x 64 blocks would be more than a sixth padding;
 * no environment variable changes it).  Outputs, each may be NULL: kernel_used (1 .. 3), opB_eff
 * (opB after the demotion of bit 1), blocks[2] = block rows and columns, grid[3] = the launch grid (x, y, z).  For a
 * Hermitian launch of kernel 1 or 2 (opB_eff bit 1) and decode != NULL: decode[3 L .. 3 L + 2] = (block row, block
 * column, batch member) of workgroup L < grid[0], or (-1, -1, -1) for a workgroup that returns at once; decode_cap
 * (in triples) below grid[0] is NEGF_EINVAL, as are the invalid arguments of negf_zgemm_batched. */
int negf_zgemm_plan(int M, int N, int K, int opB, int nb, int kernel, int* kernel_used, int* opB_eff, int* blocks,
                    int* grid, int* decode, int decode_cap);
/* What the inverse of nb matrices of dimension n launches under negf_set_inverse_algo(algo); a host function that
 * needs no device.  It is the rule the launch code itself follows (one function, k_inverse_blocked.hip); of the
 * environment only the diagnostic NEGF_GJ_STAMPS acts on it (one stream group).  defer != 0: the caller reads the reduced matrices through the
 * pivot bookkeeping (negf_gr_int does), so the windowed path leaves its gather out.  The fused kernel of n <= 96
 * (negf_set_small_algo 0) never reaches the inverse and is not part of the plan.  Outputs, each may be NULL:
 *   path      0 = no blocked kernel serves n, or algo = 1 (the unblocked kernel); 1 = the single-workgroup kernel;
 *             2 = 64-column windows
 *   nbi, rpt  path 2: the class -- sub-panel width and rows per lane of the team window kernel: (16, 1) up to n = 512,
 *             (16, 2) up to 1024, (8, 4) up to 2048, (4, 8) up to 4096, (2, 16) up to 8192
 *   nblk      path 2: windows
 *   groups    stream groups (1 .. 4; 1 for path 1, 0 for path 0); the groups tile [0, nb) in order
 *   group_tab [4][7] = per group: first, count, window kernel id, pairs (0 / 1), waves of the update launches over all
 *             other column blocks (4 = lean, 8 = fat, 0 = none), waves of the single-block update launches of a pair
 *             (0 = none), launch mask; rows from `groups` on are zero.  Window kernel ids: 1 .. 6 register-strip kernels
 *             (1 = n <= 256, 5 = 257 .. 512 lean, 6 = 513 .. 1024 eight waves; 2, 3, 4 retired variants, never answered),
 *             7 / 8 = look-ahead team kernels of 6 / 12 waves, 9 = the team kernel of the class, 10 = single workgroup.
 *             Launch mask: bit (window kernel id), bit 12 = lean update, 13 = fat update, 14 = the fused update of a
 *             pair of windows, 15 = gather
 *   gather    the gather kernel runs;  deferred: the result stays un-gathered (path 2 with defer)
 * NEGF_EINVAL: n < 1, nb < 1, algo outside 0 .. 4. */
int negf_inverse_plan(int n, int nb, int algo, int defer, int* path, int* nbi, int* rpt, int* nblk, int* groups,
                      int* group_tab, int* gather, int* deferred);
/* What the context's last inverse (dense or layered: the last layer inverted) really launched: every launch site adds
 * its bit next to its launch.  path as above (-1: no inverse yet), groups, masks[4] = the launch mask per group as in
 * negf_inverse_plan.  Each may be NULL. */
int negf_inverse_last(negf_ctx* ctx, int* path, int* groups, int* masks);

#ifdef __cplusplus
}
#endif
#endif /* NEGF_H */
