// Recursive Green's function path for layered (block-tridiagonal) devices: the negf_layered_* entry points of
// include/negf.h.  Part of negf_api.hip's translation unit (included at its end): it uses that file's allocation,
// staging and self-energy helpers as they are.
//
// A LayeredSystem is an object of its own inside the context: blocks, terminals and workspace are its own, the dense
// system (negf_set_system), its providers and its workspace are never read or written here.  What is shared is
// per-call staging with no meaning between calls: the grid / info / scalar buffers (ensure_mbuffers), the pinned host
// buffer, the Sigma kernels' scratch and the g(E) cache of the chain leads.
//
// Per energy, with C_ij = F_ij - E S_ij (the NEGATED coupling -A_ij: every sign of the textbook recursion cancels):
//   forward    g_0 = (A_00 - Sigma_left)^-1,   g_i = (A_ii - C_{i,i-1} g_{i-1} C_{i-1,i} - [i = L-1] Sigma_right)^-1
//   corner     X_0 = g_0,  X_i = g_i C_{i,i-1} X_{i-1}  -> G_{L-1,0};    Y_i = Y_{i-1} C_{i-1,i} g_i  -> G_{0,L-1}
//   backward   G_{L-1,L-1} = g_{L-1};  U = g_i C_{i,i+1},  V = C_{i+1,i} g_i:
//              G_{i,i+1} = U G_{i+1,i+1},   G_{i+1,i} = G_{i+1,i+1} V,   G_ii = g_i + G_{i,i+1} V
//   columns    of a terminal set on the union J of its orbitals (G Gamma G^H on the pattern of S), W_i = G_{i,end}[:, J]:
//              last layer:  W_{L-1} = G_{L-1,L-1}[:, J],  W_i = U_i W_{i+1}                    (backward sweep)
//              layer 0:     x_0 = g_0[:, J],  z_i = C_{i,i-1} x_{i-1},  x_i = g_i z_i          (forward sweep, the z_i kept)
//                           W_0 = G_00[:, J],  W_i = G_ii z_i                                  (backward sweep)
//              A_ii = (W_i Gamma) W_i^H,   A_{i,i+1} = (W_i Gamma) W_{i+1}^H,   A_{i+1,i} = A_{i,i+1}^H never formed
//   strips     of the transmission matrix between ALL terminals, probes on any layer included (rgf_tmat_*): with J_q the
//              union of the orbitals of the terminals on layer q,
//              strip_{L-1} = [G_{L-1,L-1}[:, J_{L-1}]],   strip_i = [G_ii[:, J_i] | U_i strip_{i+1}]   (backward sweep)
//              holds G_{i,q}[:, J_q] for every q >= i: the pairs (a on layer i, b on a layer >= i) are read from it, the
//              pairs with b on an earlier layer from the same pass over the layers in REVERSE order
// Every layer matrix of a batch is compact row-major at ONE batch stride (the largest layer's n^2): the inverses and
// products are the dense path's launchers, batched over the energies.

struct RgfTerminal {
    int end = 0;                   // 0: layer 0, 1: layer L - 1
    int kind = 0;                  // 0 const, 1 chain, 2 blocks
    int K = 0;
    int* d_idx = nullptr;          // [K] orbitals inside the layer
    std::vector<int> idx;          // the same list on the host
    int* d_pos = nullptr;          // [n_layer] position in the list, -1 outside
    cplx* d_sig = nullptr;         // const: [K*K]; blocks: [m_blk][K*K]
    int m_blk = 0;
    SigmaProvider* chain = nullptr;
    DevBuf<cplx> d_blk;            // chain: Sigma of the batch in flight [batch][K*K]
};

struct LayeredSystem {
    int L = 0, N = 0, nmax = 0;
    std::vector<int> n, off;                    // layer sizes, first orbital of each layer
    std::vector<size_t> doff, uoff;             // start of diagonal block i / coupling block (i, i+1) in the flat arrays
    size_t dtot = 0, utot = 0;
    cplx *dFd = nullptr, *dSd = nullptr;        // diagonal blocks
    cplx *dFu = nullptr, *dSu = nullptr;        // upper blocks (i, i+1), n_i x n_{i+1}
    cplx *dFl = nullptr, *dSl = nullptr;        // lower blocks (i+1, i) = their conjugate transposes, n_{i+1} x n_i
    std::vector<RgfTerminal*> terms;
    size_t stride = 0;                          // elements between the matrices of a batch
    DevBuf<cplx> d_pool;                        // [RGF_NBUF][batch][stride] work areas
    DevBuf<cplx> d_gstore;                      // [L][batch][stride] the g_i of a backward sweep
    DevBuf<cplx> d_small;                       // Gamma_a | Gamma_b | G_ab | X | Y of the transmission
    DevBuf<cplx> d_cols;                        // column sets of G Gamma G^H: z_i | x | W | Y | Gamma, per energy in flight;
                                                // of a transmission matrix: strip | strip | Gamma(E) | G_ab | X | Y
    DevBuf<int> d_J;                            // [2][nmax] their union lists, layer 0's then the last layer's
    DevBuf<cplx> d_out;                         // gr_int: the block lists, host-pointer entry point
    DevBuf<double> d_site;                      // dos: [m][N] staging of the host-pointer entry point
    DevBuf<int> d_tm_tab;                       // transmission matrix: the terminal tables, union lists and pair lists
    DevBuf<cplx> d_tm_sig, d_tm_gam;            // ... the probes' Sigma blocks; the Gamma blocks that do not depend on E
    DevBuf<int> d_piv, d_linfo, d_iters, d_conv;
    int batch = 0;                              // energies the work areas are laid out for
    long long work_bytes = 0;                   // of the last call: pool + stored g + column sets
};

constexpr int RGF_NBUF = 10;

static void free_terminal(RgfTerminal* t)
{
    if (!t) return;
    dev_free(t->d_idx); dev_free(t->d_pos); dev_free(t->d_sig);
    release_bufs(t->d_blk);
    if (t->chain) free_provider(t->chain);
    delete t;
}

void free_layered(LayeredSystem* ls)
{
    if (!ls) return;
    for (auto* t : ls->terms) free_terminal(t);
    dev_free(ls->dFd); dev_free(ls->dSd); dev_free(ls->dFu); dev_free(ls->dSu); dev_free(ls->dFl); dev_free(ls->dSl);
    release_bufs(ls->d_pool, ls->d_gstore, ls->d_small, ls->d_out, ls->d_cols);
    release_bufs(ls->d_site);
    release_bufs(ls->d_J, ls->d_tm_tab);
    release_bufs(ls->d_tm_sig, ls->d_tm_gam);
    release_bufs(ls->d_piv, ls->d_linfo, ls->d_iters, ls->d_conv);
    delete ls;
}

namespace {

LayeredSystem* get_layered(negf_ctx* c, int handle)
{
    if (!c || handle < 0 || handle >= (int)c->layered.size()) return nullptr;
    return c->layered[handle];
}

// the index list of a terminal: inside its layer, no orbital twice
bool rgf_valid_list(int n, int K, const int* inds)
{
    if (K < 1 || K > n || !inds) return false;
    std::vector<char> seen((size_t)n, 0);
    for (int a = 0; a < K; ++a) {
        if (inds[a] < 0 || inds[a] >= n || seen[inds[a]]) return false;
        seen[inds[a]] = 1;
    }
    return true;
}

// Opens a terminal on layer `layer` (0 or L - 1) of system h; validation only, nothing launched
int rgf_new_terminal(negf_ctx* c, int h, int layer, int K, const int* inds, int* terminal, LayeredSystem** lsp, RgfTerminal** tp)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls || !terminal) return NEGF_EINVAL;
    if (layer != 0 && layer != ls->L - 1) return NEGF_EINVAL;              // interior layers carry no terminal
    const int end = layer == 0 ? 0 : 1;
    const int nl = ls->n[layer];
    if (!rgf_valid_list(nl, K, inds)) return NEGF_EINVAL;
    int on_end = 0;
    for (auto* t : ls->terms) on_end += t->end == end;
    if (on_end >= RGF_MAX_TERM) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    RgfTerminal* t = new RgfTerminal();
    t->end = end; t->K = K;
    t->idx.assign(inds, inds + K);
    std::vector<int> pos((size_t)nl, -1);
    for (int a = 0; a < K; ++a) pos[inds[a]] = a;
    int rc;
    if ((rc = dev_alloc(&t->d_idx, (size_t)K)) || (rc = dev_alloc(&t->d_pos, (size_t)nl)) ||
        (rc = upload(c, t->d_idx, inds, (size_t)K)) || (rc = upload(c, t->d_pos, pos.data(), (size_t)nl))) { free_terminal(t); return rc; }
    *lsp = ls; *tp = t;
    return NEGF_OK;
}

int rgf_add_terminal(LayeredSystem* ls, RgfTerminal* t) { ls->terms.push_back(t); return (int)ls->terms.size() - 1; }

// A G Gamma G^H call: the terminals it selects, per end (0: layer 0, 1: layer L - 1) the union J of their orbitals, and
// the column areas of the batch in flight (all compact n_i x K at the stride cs)
typedef void (*RgfConsumeA)(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* A, bool up, void* arg);
struct RgfLess {
    int K[2] = {0, 0};                          // |J|, 0: no terminal of that end selected
    const int* J[2] = {nullptr, nullptr};       // device, ascending
    const RgfTerminal* only = nullptr;          // the one terminal selected, null: all
    size_t cs = 0, per_energy = 0;
    cplx *z = nullptr, *x[2] = {nullptr, nullptr};          // layer-0 set: z_1 .. z_{L-1} [L-1][batch][cs], x_{i-1} | x_i
    cplx *W[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *Y[2] = {nullptr, nullptr}, *gam[2] = {nullptr, nullptr};
    RgfConsumeA consume = nullptr; void* arg = nullptr;
};

struct RgfRun {
    LayeredSystem* ls;
    int nb_max;                 // energies per sweep
    cplx* buf[RGF_NBUF];
};

// Energies per sweep and the work areas for them.  A sweep holds RGF_NBUF matrices of the largest layer per energy, a
// backward sweep L more (the g_i), a G Gamma G^H call `extra` elements more (its column sets, rgf_less_layout); the budget
// is the dense path's (auto_batch): a quarter of the free HBM, at most 64 GB.
int rgf_workspace(negf_ctx* c, LayeredSystem* ls, int m, bool backward, RgfRun* r, size_t extra = 0)
{
    const size_t s = ls->stride;
    const int nbufs = RGF_NBUF + (backward ? ls->L : 0);
    int want;
    if (c->batch_user > 0) want = std::min(c->batch_user, std::max(m, 1));
    else {
        const double per = 16.0 * ((double)s * nbufs + (double)extra);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)24e9;
        // (what this system already holds counts as free: it is reused)
        const double held = 16.0 * (double)(ls->d_pool.cap + ls->d_gstore.cap + ls->d_cols.cap);
        const double budget = std::min(64.0e9, std::max(2.0e9, 0.25 * ((double)free_b + held)));
        long b = (long)(budget / per);
        b = std::max(1L, std::min(b, 4096L));
        want = (int)std::min<long>(b, std::max(m, 1));
    }
    int rc;
    if ((rc = ensure_cap(c, ls->d_pool, (size_t)RGF_NBUF * want * s + 64))) return rc;
    if (backward && (rc = ensure_cap(c, ls->d_gstore, (size_t)ls->L * want * s + 64))) return rc;
    if (extra && (rc = ensure_cap(c, ls->d_cols, extra * want + 64))) return rc;
    if ((rc = ensure_cap(c, ls->d_piv, (size_t)2 * ls->nmax * want)) || (rc = ensure_cap(c, ls->d_linfo, (size_t)want)) ||
        (rc = ensure_cap(c, ls->d_iters, (size_t)want)) || (rc = ensure_cap(c, ls->d_conv, (size_t)want))) return rc;
    for (auto* t : ls->terms)
        if (t->kind == 1 && (rc = ensure_cap(c, t->d_blk, (size_t)want * t->K * t->K))) return rc;
    ls->batch = want;
    ls->work_bytes = 16LL * ((long long)s * nbufs + (long long)extra) * want;
    r->ls = ls; r->nb_max = want;
    for (int k = 0; k < RGF_NBUF; ++k) r->buf[k] = ls->d_pool + (size_t)k * want * s;
    return NEGF_OK;
}

// What every call checks before it launches anything
int rgf_open(negf_ctx* c, int h, int m, LayeredSystem** lsp)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls || m < 0) return NEGF_EINVAL;
    for (auto* t : ls->terms) if (t->kind == 2 && m > t->m_blk) return NEGF_EINVAL;   // more energies than Sigma blocks supplied
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    *lsp = ls;
    return NEGF_OK;
}

// Sigma blocks of the chain terminals for the energies [m0, m0 + nb) -> their d_blk
int rgf_chain_sigmas(negf_ctx* c, LayeredSystem* ls, int m0, int nb, const cplx* E)
{
    for (auto* t : ls->terms) {
        if (t->kind != 1) continue;
        int rc = run_sigma_blocks(c, t->chain, nb, E + m0, ls->d_iters, ls->d_conv, m0, t->d_blk.p);
        if (rc) return rc;
    }
    return NEGF_OK;
}

// where terminal t's Sigma of the batch starting at m0 lies, and its stride over the energies
void rgf_sigma_of(const RgfTerminal* t, int m0, const cplx** sig, size_t* stride)
{
    const size_t kk = (size_t)t->K * t->K;
    if (t->kind == 0) { *sig = t->d_sig; *stride = 0; }
    else if (t->kind == 2) { *sig = t->d_sig + kk * m0; *stride = kk; }
    else { *sig = t->d_blk.p; *stride = kk; }
}

// (only: the one terminal that counts, null: all of that end)
RgfTermArgs rgf_term_args(const LayeredSystem* ls, int end, int m0, const RgfTerminal* only = nullptr)
{
    RgfTermArgs a;
    for (int k = 0; k < RGF_MAX_TERM; ++k) { a.pos[k] = nullptr; a.sig[k] = nullptr; a.stride[k] = 0; a.K[k] = 0; }
    for (auto* t : ls->terms) {
        if (t->end != end || (only && t != only)) continue;
        const int k = a.count++;
        a.pos[k] = t->d_pos; a.K[k] = t->K;
        rgf_sigma_of(t, m0, &a.sig[k], &a.stride[k]);
    }
    return a;
}

// D[b] = A_ii(E_b) - P[b] - the terminals of layer i
void rgf_assemble_diag(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* E, const cplx* P, cplx* D)
{
    ProfScope ps(c, "rgf");
    RgfTermArgs ta;
    if (i == 0) ta = rgf_term_args(ls, 0, m0);
    else if (i == ls->L - 1) ta = rgf_term_args(ls, 1, m0);
    else ta = rgf_term_args(ls, -1, m0);
    launch_rgf_diag(c->stream, ls->n[i], nb, E + m0, ls->dSd + ls->doff[i], ls->dFd + ls->doff[i], P, ls->stride, ta, D, ls->stride);
}

// the negated couplings of the pair (i, i+1): CU = C_{i,i+1} (n_i x n_{i+1}), CL = C_{i+1,i}
void rgf_couplings(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* E, cplx* CU, cplx* CL)
{
    ProfScope ps(c, "rgf");
    const int cnt = ls->n[i] * ls->n[i + 1];
    launch_rgf_coupling(c->stream, cnt, nb, E + m0, ls->dSu + ls->uoff[i], ls->dFu + ls->uoff[i], CU, ls->stride);
    launch_rgf_coupling(c->stream, cnt, nb, E + m0, ls->dSl + ls->uoff[i], ls->dFl + ls->uoff[i], CL, ls->stride);
}

// C[b] (M x N) = A[b] (M x K) B[b] (K x N), all compact at the system's stride
void rgf_mm(negf_ctx* c, LayeredSystem* ls, int M, int N, int K, int nb, const cplx* A, const cplx* B, cplx* C)
{
    ProfScope ps(c, "zgemm");
    launch_zgemm(c->stream, M, N, K, nb, A, K, ls->stride, B, N, ls->stride, 0, C, N, ls->stride);
}

// In-place inverse of the n x n matrices in A with B as the blocked kernels' second area: *res = where the inverses
// lie.  A zero pivot of layer i is reported as column off_i + k of the whole system.
int rgf_inverse(negf_ctx* c, LayeredSystem* ls, int i, int nb, cplx* A, cplx* B, int* info, cplx** res)
{
    const int n = ls->n[i];
    {
        ProfScope ps(c, "inverse");
        int algo = c->inverse_algo;
        if (algo == 0) algo = inverse_blocked_supported(n) ? 2 : 1;
        const int win_mode = algo == 3 ? 1 : algo == 4 ? 2 : 0;
        if (algo > 2) algo = 2;
        bool in_b = false;
        if (algo == 2) {
            in_b = launch_inverse_blocked(c->stream, n, nb, A, B, ls->stride, ls->d_piv, ls->d_linfo, &c->gj_side, win_mode, nullptr);
            if (!in_b) algo = 1;
        }
        if (algo == 1 && !launch_inverse_unblocked(c->stream, n, nb, A, ls->d_linfo, ls->stride)) return NEGF_EINVAL;
        NEGF_HIP_CHECK(hipGetLastError());
        const double dn = n, np = (double)((n + 15) & ~15), k4 = (double)((n + 3) & ~3);
        negf_count_flops(8.0 * dn * dn * dn * nb, algo == 2 ? 6.0 * np * np * k4 * nb - inverse_blocked_vector_flops() : 0.0);
        *res = in_b ? B : A;
    }
    launch_rgf_merge_info(c->stream, nb, ls->off[i], ls->d_linfo, info);
    return NEGF_OK;
}

// Forward sweep of the batch [m0, m0 + nb).  keep: the g_i go to d_gstore (a backward sweep follows); otherwise only
// g_{i-1} is alive, and the corner block X_i (corner = 1: G_{i,0}) or Y_i (corner = 2: G_{0,i}) is carried along --
// *corner_out = the block of the last layer.  less (with keep): the z_i chain of a column set on layer 0.  Work areas:
// buf[0..8].
int rgf_forward(negf_ctx* c, const RgfRun& r, int m0, int nb, const cplx* E, bool keep, int corner, cplx** corner_out,
                RgfLess* less = nullptr)
{
    LayeredSystem* ls = r.ls;
    const size_t s = ls->stride;
    const size_t layer_bytes = (size_t)nb * s * sizeof(cplx);
    cplx *CU = r.buf[0], *CL = r.buf[1], *T = r.buf[2], *P = r.buf[3];
    cplx* R[3] = {r.buf[4], r.buf[5], r.buf[6]};           // rotating: g_{i-1} | matrix to invert | second area
    cplx *Xa = r.buf[7], *Xb = r.buf[8];
    int* info = c->d_info + m0;
    NEGF_HIP_CHECK(hipMemsetAsync(info, 0, (size_t)nb * sizeof(int), c->stream));
    int rc;
    if ((rc = rgf_chain_sigmas(c, ls, m0, nb, E))) return rc;
    cplx* gprev = nullptr;
    for (int i = 0; i < ls->L; ++i) {
        const int ni = ls->n[i];
        cplx *D, *B;
        if (keep) { D = ls->d_gstore + (size_t)i * r.nb_max * s; B = R[0]; }
        else {
            cplx* fr[3]; int k = 0;
            for (cplx* q : R) if (q != gprev) fr[k++] = q;             // the two areas g_{i-1} does not occupy
            D = fr[0]; B = fr[1];
        }
        if (i > 0) {
            const int np = ls->n[i - 1];
            rgf_couplings(c, ls, i - 1, m0, nb, E, CU, CL);
            rgf_mm(c, ls, ni, np, np, nb, CL, gprev, T);               // C_{i,i-1} g_{i-1}
            rgf_mm(c, ls, ni, ni, np, nb, T, CU, P);                   // ... C_{i-1,i}
        }
        rgf_assemble_diag(c, ls, i, m0, nb, E, i > 0 ? P : nullptr, D);
        cplx* g = nullptr;
        if ((rc = rgf_inverse(c, ls, i, nb, D, B, info, &g))) return rc;
        if (keep && g != D) { NEGF_HIP_CHECK(hipMemcpyAsync(D, g, layer_bytes, hipMemcpyDeviceToDevice, c->stream)); g = D; }
        if (keep && less && less->K[0] > 0) {
            const int K = less->K[0];
            if (i == 0) { ProfScope ps(c, "rgf"); launch_rgf_gather_cols(c->stream, ni, K, nb, g, s, less->J[0], less->x[0], less->cs); }
            else {
                cplx* z = less->z + (size_t)(i - 1) * r.nb_max * less->cs;
                ProfScope ps(c, "zgemm");
                launch_zgemm(c->stream, ni, K, ls->n[i - 1], nb, CL, ls->n[i - 1], s, less->x[0], K, less->cs, 0, z, K, less->cs);   // z_i = C_{i,i-1} x_{i-1}
                if (i + 1 < ls->L) {
                    launch_zgemm(c->stream, ni, K, ni, nb, g, ni, s, z, K, less->cs, 0, less->x[1], K, less->cs);                 // x_i = g_i z_i
                    std::swap(less->x[0], less->x[1]);
                }
            }
        }
        if (!keep && corner) {
            const int n0 = ls->n[0];
            if (i == 0) { NEGF_HIP_CHECK(hipMemcpyAsync(Xa, g, layer_bytes, hipMemcpyDeviceToDevice, c->stream)); }
            else if (corner == 1) {
                rgf_mm(c, ls, ni, n0, ls->n[i - 1], nb, CL, Xa, T);    // C_{i,i-1} X_{i-1}
                rgf_mm(c, ls, ni, n0, ni, nb, g, T, Xb);               // X_i = g_i ...
                std::swap(Xa, Xb);
            } else {
                rgf_mm(c, ls, n0, ni, ls->n[i - 1], nb, Xa, CU, T);    // Y_{i-1} C_{i-1,i}
                rgf_mm(c, ls, n0, ni, ni, nb, T, g, Xb);               // Y_i = ... g_i
                std::swap(Xa, Xb);
            }
        }
        gprev = g;
    }
    if (corner_out) *corner_out = Xa;
    return NEGF_OK;
}

// what a backward sweep hands to its consumer, layer by layer from the last one down: G_ii, and for i < L - 1 the
// blocks G_{i,i+1}, G_{i+1,i} (null for the last layer)
typedef void (*RgfConsume)(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* Gii, const cplx* Gup, const cplx* Glo, void* arg);

// Layer i of a G Gamma G^H sweep: the columns W_i of each selected end from G_ii, U_i and W_{i+1}, then the blocks A_ii and
// A_{i,i+1} (the layer-0 set's contribution first, the last layer's added to it) handed to the consumer one after the other.
// Work areas: buf[9], buf[4], buf[3] -- free once G_ii stands.
void rgf_less_layer(negf_ctx* c, const RgfRun& r, RgfLess* less, int i, int m0, int nb, const cplx* Gii, const cplx* U)
{
    LayeredSystem* ls = r.ls;
    const size_t s = ls->stride, cs = less->cs;
    const int ni = ls->n[i], L = ls->L;
    for (int e = 0; e < 2; ++e) {
        const int K = less->K[e];
        if (K == 0) continue;
        cplx* W = less->W[e][1];
        if ((e == 0 && i == 0) || (e == 1 && i == L - 1)) {
            ProfScope ps(c, "rgf");
            launch_rgf_gather_cols(c->stream, ni, K, nb, Gii, s, less->J[e], W, cs);
        } else if (e == 0) {
            ProfScope ps(c, "zgemm");
            launch_zgemm(c->stream, ni, K, ni, nb, Gii, ni, s, less->z + (size_t)(i - 1) * r.nb_max * cs, K, cs, 0, W, K, cs);    // G_ii z_i
        } else {
            const int nn = ls->n[i + 1];
            ProfScope ps(c, "zgemm");
            launch_zgemm(c->stream, ni, K, nn, nb, U, nn, s, less->W[e][0], K, cs, 0, W, K, cs);                                 // U_i W_{i+1}
        }
        ProfScope ps(c, "zgemm");
        launch_zgemm(c->stream, ni, K, K, nb, W, K, cs, less->gam[e], K, (size_t)K * K, 0, less->Y[e], K, cs);                   // Y_i = W_i Gamma
    }
    cplx* Ab[2] = {r.buf[9], r.buf[4]};
    const bool both = less->K[0] > 0 && less->K[1] > 0;
    for (int up = 0; up < 2; ++up) {
        if (up && i == L - 1) break;
        const int nc = up ? ls->n[i + 1] : ni;
        for (int e = 0; e < 2; ++e) {
            const int K = less->K[e];
            if (K == 0) continue;
            ProfScope ps(c, "zgemm");
            // op(B) = W^H; the diagonal block is a Hermitian product
            launch_zgemm(c->stream, ni, nc, K, nb, less->Y[e], K, cs, less->W[e][up ? 0 : 1], K, cs, up ? 1 : 3, Ab[e], nc, s);
        }
        const cplx* A = less->K[0] > 0 ? Ab[0] : Ab[1];
        if (both) { ProfScope ps(c, "rgf"); launch_rgf_add(c->stream, ni * nc, nb, Ab[0], s, Ab[1], s, r.buf[3], s); A = r.buf[3]; }
        less->consume(c, ls, i, m0, nb, A, up != 0, less->arg);
    }
    for (int e = 0; e < 2; ++e) std::swap(less->W[e][0], less->W[e][1]);       // W_i is the next layer's W_{i+1}
}

// less: a G Gamma G^H sweep -- the consumer is less->consume (consume is null), G_{i+1,i} is not formed
int rgf_backward(negf_ctx* c, const RgfRun& r, int m0, int nb, const cplx* E, RgfConsume consume, void* arg, RgfLess* less = nullptr)
{
    LayeredSystem* ls = r.ls;
    const size_t s = ls->stride;
    cplx *CU = r.buf[0], *CL = r.buf[1], *U = r.buf[2], *V = r.buf[3], *Wm = r.buf[4], *Gup = r.buf[5], *Glo = r.buf[6];
    cplx *Gcur = r.buf[7], *Galt = r.buf[8];
    auto g_of = [&](int i) { return ls->d_gstore + (size_t)i * r.nb_max * s; };
    const cplx* Gnext = g_of(ls->L - 1);
    if (less) rgf_less_layer(c, r, less, ls->L - 1, m0, nb, Gnext, nullptr);
    else consume(c, ls, ls->L - 1, m0, nb, Gnext, nullptr, nullptr, arg);
    for (int i = ls->L - 2; i >= 0; --i) {
        const int ni = ls->n[i], nn = ls->n[i + 1];
        const cplx* g = g_of(i);
        rgf_couplings(c, ls, i, m0, nb, E, CU, CL);
        rgf_mm(c, ls, ni, nn, ni, nb, g, CU, U);                       // U = g_i C_{i,i+1}
        rgf_mm(c, ls, ni, nn, nn, nb, U, Gnext, Gup);                  // G_{i,i+1}
        rgf_mm(c, ls, nn, ni, ni, nb, CL, g, V);                       // V = C_{i+1,i} g_i
        if (!less) rgf_mm(c, ls, nn, ni, nn, nb, Gnext, V, Glo);       // G_{i+1,i}
        rgf_mm(c, ls, ni, ni, nn, nb, Gup, V, Wm);                     // g_i C G_{i+1,i+1} C g_i
        { ProfScope ps(c, "rgf"); launch_rgf_add(c->stream, ni * ni, nb, g, s, Wm, s, Gcur, s); }
        if (less) rgf_less_layer(c, r, less, i, m0, nb, Gcur, U);
        else consume(c, ls, i, m0, nb, Gcur, Gup, Glo, arg);
        Gnext = Gcur;
        std::swap(Gcur, Galt);
    }
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

struct RgfDosArg { int form; double* site; };      // site: [m][N] on the device

void rgf_consume_dos(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* Gii, const cplx* Gup, const cplx* Glo, void* arg)
{
    ProfScope ps(c, "rgf");
    const RgfDosArg* a = static_cast<const RgfDosArg*>(arg);
    const size_t s = ls->stride;
    double* site = a->site + (size_t)m0 * ls->N;
    if (a->form == 0) { launch_rgf_dos_diag(c->stream, ls->n[i], nb, Gii, s, site + ls->off[i], (size_t)ls->N); return; }
    // -Im (G S)_rr / pi, S_kr read as conj(S_rk): the diagonal block, then the two neighbours
    launch_rgf_dos_rows(c->stream, ls->n[i], ls->n[i], nb, Gii, s, ls->dSd + ls->doff[i], site + ls->off[i], (size_t)ls->N, false);
    if (Gup) {
        launch_rgf_dos_rows(c->stream, ls->n[i], ls->n[i + 1], nb, Gup, s, ls->dSu + ls->uoff[i], site + ls->off[i], (size_t)ls->N, true);
        launch_rgf_dos_rows(c->stream, ls->n[i + 1], ls->n[i], nb, Glo, s, ls->dSl + ls->uoff[i], site + ls->off[i + 1], (size_t)ls->N, true);
    }
}

struct RgfSumArg { const cplx* w; cplx* out; };

void rgf_consume_sum(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* Gii, const cplx* Gup, const cplx* Glo, void* arg)
{
    ProfScope ps(c, "accumulate");
    const RgfSumArg* a = static_cast<const RgfSumArg*>(arg);
    const size_t s = ls->stride;
    launch_rgf_accumulate(c->stream, ls->n[i] * ls->n[i], nb, a->w + m0, Gii, s, a->out + ls->doff[i]);
    if (Gup) {
        const int cnt = ls->n[i] * ls->n[i + 1];
        launch_rgf_accumulate(c->stream, cnt, nb, a->w + m0, Gup, s, a->out + ls->dtot + ls->uoff[i]);
        launch_rgf_accumulate(c->stream, cnt, nb, a->w + m0, Glo, s, a->out + ls->dtot + ls->utot + ls->uoff[i]);
    }
}

bool rgf_less_ind_ok(const LayeredSystem* ls, int ind)
{
    const int nt = (int)ls->terms.size();
    return ind == NEGF_IND_TOTAL ? nt > 0 : (ind >= -nt && ind < nt);
}

// Which terminals `ind` names (negf_gless_int's reading: -n_t .. n_t - 1, NEGF_IND_TOTAL = all), their union lists on
// the device, and the size of the column areas per energy.  NEGF_EINVAL before anything is launched.
int rgf_less_select(negf_ctx* c, LayeredSystem* ls, int ind, RgfLess* less)
{
    if (!rgf_less_ind_ok(ls, ind)) return NEGF_EINVAL;
    if (ind != NEGF_IND_TOTAL) less->only = ls->terms[ind < 0 ? ind + (int)ls->terms.size() : ind];
    std::vector<int> J[2];
    for (int e = 0; e < 2; ++e) {
        const int nl = ls->n[e == 0 ? 0 : ls->L - 1];
        std::vector<char> in((size_t)nl, 0);
        for (auto* t : ls->terms)
            if (t->end == e && (!less->only || t == less->only)) for (int o : t->idx) in[o] = 1;
        for (int o = 0; o < nl; ++o) if (in[o]) J[e].push_back(o);
        less->K[e] = (int)J[e].size();
    }
    int rc;
    if ((rc = ensure_cap(c, ls->d_J, (size_t)2 * ls->nmax))) return rc;
    for (int e = 0; e < 2; ++e) {
        less->J[e] = ls->d_J + (size_t)e * ls->nmax;
        if ((rc = upload(c, ls->d_J + (size_t)e * ls->nmax, J[e].data(), J[e].size()))) return rc;
    }
    const size_t Kmax = (size_t)std::max(less->K[0], less->K[1]);
    less->cs = (size_t)ls->nmax * Kmax;
    // layer-0 set: z_1 .. z_{L-1}, x | x, W | W, Y;  last layer's: W | W, Y;  and the two Gamma
    less->per_energy = (less->K[0] > 0 ? (size_t)(ls->L - 1) + 5 : 0) * less->cs + (less->K[1] > 0 ? 3 : 0) * less->cs +
                       (size_t)less->K[0] * less->K[0] + (size_t)less->K[1] * less->K[1];
    return NEGF_OK;
}

// carve the column areas out of d_cols for the batch size of this run
void rgf_less_layout(const RgfRun& r, RgfLess* less)
{
    const size_t cb = less->cs * r.nb_max;
    cplx* p = r.ls->d_cols.p;
    auto take = [&](size_t count) { cplx* q = p; p += count; return q; };
    if (less->K[0] > 0) {
        less->z = take((size_t)(r.ls->L - 1) * cb);
        less->x[0] = take(cb); less->x[1] = take(cb);
    }
    for (int e = 0; e < 2; ++e) {
        if (less->K[e] == 0) continue;
        less->W[e][0] = take(cb); less->W[e][1] = take(cb); less->Y[e] = take(cb);
        less->gam[e] = take((size_t)less->K[e] * less->K[e] * r.nb_max);
    }
}

// forward sweep, the Gamma of the selected terminals on their union lists, backward sweep of one batch
int rgf_less_batch(negf_ctx* c, const RgfRun& r, RgfLess* less, int m0, int nb, const cplx* E)
{
    int rc;
    if ((rc = rgf_forward(c, r, m0, nb, E, true, 0, nullptr, less))) return rc;
    {
        ProfScope ps(c, "gamma");
        for (int e = 0; e < 2; ++e)
            if (less->K[e] > 0)
                launch_rgf_gamma_union(c->stream, less->K[e], nb, less->J[e], rgf_term_args(r.ls, e, m0, less->only), less->gam[e],
                                       (size_t)less->K[e] * less->K[e]);
    }
    return rgf_backward(c, r, m0, nb, E, nullptr, nullptr, less);
}

void rgf_consume_less_sum(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* A, bool up, void* arg)
{
    ProfScope ps(c, "accumulate");
    const RgfSumArg* a = static_cast<const RgfSumArg*>(arg);
    const size_t s = ls->stride;
    if (!up) { launch_rgf_accumulate(c->stream, ls->n[i] * ls->n[i], nb, a->w + m0, A, s, a->out + ls->doff[i]); return; }
    launch_rgf_accumulate(c->stream, ls->n[i] * ls->n[i + 1], nb, a->w + m0, A, s, a->out + ls->dtot + ls->uoff[i]);
    // the lower block (i+1, i): sum_k w_k conj(A_{i,i+1}(E_k))^T
    launch_rgf_accumulate_ct(c->stream, ls->n[i], ls->n[i + 1], nb, a->w + m0, A, s, a->out + ls->dtot + ls->utot + ls->uoff[i]);
}

void rgf_consume_less_dos(negf_ctx* c, LayeredSystem* ls, int i, int m0, int nb, const cplx* A, bool up, void* arg)
{
    ProfScope ps(c, "rgf");
    double* site = static_cast<double*>(arg) + (size_t)m0 * ls->N;
    const size_t s = ls->stride;
    if (!up) launch_rgf_pop_block(c->stream, ls->n[i], ls->n[i], nb, A, s, ls->dSd + ls->doff[i], site + ls->off[i], false, nullptr, (size_t)ls->N);
    // the rows of layer i, and through A_{i+1,i} = A_{i,i+1}^H the rows of layer i + 1 as the block's column sums
    else launch_rgf_pop_block(c->stream, ls->n[i], ls->n[i + 1], nb, A, s, ls->dSu + ls->uoff[i], site + ls->off[i], true,
                              site + ls->off[i + 1], (size_t)ls->N);
}

// ------------------------------------------------- transmission matrix between all terminals, probes on any layer
// Terminals: the system's end terminals in the order they were made, then the call's probes (orbital lists numbered in
// the whole system, each inside ONE layer).  Two passes of forward sweep (g_i kept) and backward sweep with column strips:
// pass 0 over the layers as they are serves the pairs (a, b) with layer(b) >= layer(a), pass 1 over the layers in reverse
// order (view level i = layer L - 1 - i, C_{i,i+1} and C_{i+1,i} swapped -- a view, no block is copied) the others.
struct RgfTmatPlan {
    int C = 0, nt = 0, n_probes = 0, Ktot = 0;
    std::vector<int> K, layer, ioff, goff, gstride, soff;      // per terminal
    std::vector<int> tcol[2];                                  // first strip column of the terminal's layer, per pass
    std::vector<int> rows, cpos;                               // per terminal orbital: index inside its layer, position in J
    std::vector<int> nJ, Joff, J;                              // per layer: |J_q|, start in J; the union lists, ascending
    std::vector<int> colbase[2];                               // per layer and pass: columns of the layers before it in view
    std::vector<int> porder, poff;                             // the probes of layer q in content order: porder[poff[q] .. poff[q+1])
    std::vector<int> pairs;                                    // a * C + b, grouped by (pass, level, class)
    std::vector<int> pair_at, pair_n;                          // [(pass * L + level) * 3 + class]
    int max_elems[3] = {0, 0, 0};
    size_t psum = 0, stat = 0, dyn = 0, big_kk = 0;            // sum K_p^2 | static Gamma elements | per-energy ones | class 0
    bool two_pass = false;
    // device tables
    const int *dK = nullptr, *d_ioff = nullptr, *d_goff = nullptr, *d_gstride = nullptr, *d_soff = nullptr;
    const int *d_tcol[2] = {nullptr, nullptr}, *d_rows = nullptr, *d_cpos = nullptr, *d_J = nullptr, *d_porder = nullptr;
    const int* d_pairs = nullptr;
    // work areas of the batch in flight
    size_t cs = 0, per_energy = 0;
    cplx *strip[2] = {nullptr, nullptr}, *gdyn = nullptr, *Gab = nullptr, *Xs = nullptr, *Ys = nullptr;
};

// validation and the host tables; NEGF_EINVAL before anything is launched
int rgf_tmat_plan(LayeredSystem* ls, int n_probes, const int* probe_nk, const int* probe_inds, const cplx* psig, RgfTmatPlan* pl)
{
    if (n_probes < 0 || (n_probes > 0 && (!probe_nk || !probe_inds || !psig))) return NEGF_EINVAL;
    const int L = ls->L, nt = (int)ls->terms.size();
    if ((long)nt + n_probes > TMAT_MAX_TERMINALS || nt + n_probes == 0) return NEGF_EINVAL;
    const int C = nt + n_probes;
    pl->C = C; pl->nt = nt; pl->n_probes = n_probes;
    pl->K.resize(C); pl->layer.resize(C); pl->ioff.resize(C); pl->goff.resize(C); pl->gstride.resize(C); pl->soff.assign(C, 0);
    for (int t = 0; t < nt; ++t) {
        const RgfTerminal* T = ls->terms[t];
        pl->K[t] = T->K; pl->layer[t] = T->end == 0 ? 0 : L - 1; pl->ioff[t] = (int)pl->rows.size();
        pl->rows.insert(pl->rows.end(), T->idx.begin(), T->idx.end());
    }
    std::vector<char> seen((size_t)ls->N, 0);
    size_t isum = 0, psum = 0;
    for (int q = 0; q < n_probes; ++q) {
        const int t = nt + q, k = probe_nk[q];
        if (k < 1) return NEGF_EINVAL;
        const int* I = probe_inds + isum;
        int lay = -1;
        for (int i = 0; i < k; ++i) {
            const int v = I[i];
            if (v < 0 || v >= ls->N || seen[v]) return NEGF_EINVAL;
            seen[v] = 1;
            const int l = (int)(std::upper_bound(ls->off.begin(), ls->off.end(), v) - ls->off.begin()) - 1;
            if (lay >= 0 && l != lay) return NEGF_EINVAL;                  // a probe lives on one layer
            lay = l;
        }
        for (int i = 0; i < k; ++i) seen[I[i]] = 0;
        pl->K[t] = k; pl->layer[t] = lay; pl->ioff[t] = (int)pl->rows.size(); pl->soff[t] = (int)psum;
        for (int i = 0; i < k; ++i) pl->rows.push_back(I[i] - ls->off[lay]);
        isum += k; psum += (size_t)k * k;
        if (psum > ((size_t)1 << 30)) return NEGF_EINVAL;
    }
    pl->psum = psum;
    // Gamma blocks: the probes' (at their Sigma's offsets) and the const terminals' once per call, the others per energy
    size_t stat = psum, dyn = 0;
    for (int t = 0; t < nt; ++t) {
        const size_t kk = (size_t)pl->K[t] * pl->K[t];
        if (ls->terms[t]->kind == 0) { pl->goff[t] = (int)stat; stat += kk; }
        else { pl->goff[t] = (int)dyn; dyn += kk; }
    }
    for (int t = 0; t < nt; ++t) pl->gstride[t] = ls->terms[t]->kind == 0 ? 0 : (int)dyn;
    for (int t = nt; t < C; ++t) { pl->goff[t] = pl->soff[t]; pl->gstride[t] = 0; }
    pl->stat = stat; pl->dyn = dyn;
    // union lists J_q and every terminal orbital's position in its layer's list
    pl->nJ.assign(L, 0); pl->Joff.assign(L, 0);
    std::vector<std::vector<int>> on(L);
    for (int t = 0; t < C; ++t) on[pl->layer[t]].push_back(t);
    pl->cpos.assign(pl->rows.size(), 0);
    int first = L, last = -1;
    for (int q = 0; q < L; ++q) {
        pl->Joff[q] = (int)pl->J.size();
        if (on[q].empty()) continue;
        first = std::min(first, q); last = std::max(last, q);
        std::vector<int> pos((size_t)ls->n[q], -1);
        for (int t : on[q]) for (int i = 0; i < pl->K[t]; ++i) pos[pl->rows[pl->ioff[t] + i]] = 0;
        int cnt = 0;
        for (int o = 0; o < ls->n[q]; ++o) if (pos[o] == 0) { pos[o] = cnt++; pl->J.push_back(o); }
        pl->nJ[q] = cnt;
        for (int t : on[q]) for (int i = 0; i < pl->K[t]; ++i) pl->cpos[pl->ioff[t] + i] = pos[pl->rows[pl->ioff[t] + i]];
    }
    pl->Ktot = (int)pl->J.size();
    pl->two_pass = first != last;
    for (int pass = 0; pass < 2; ++pass) {
        pl->colbase[pass].assign(L, 0);
        int acc = 0;
        for (int i = 0; i < L; ++i) { const int p = pass ? L - 1 - i : i; pl->colbase[pass][p] = acc; acc += pl->nJ[p]; }
        pl->tcol[pass].resize(C);
        for (int t = 0; t < C; ++t) pl->tcol[pass][t] = pl->colbase[pass][pl->layer[t]];
    }
    // the probes of each layer in content order: tmat_plan's comparison (size, orbital list, the block's values as numbers)
    pl->poff.assign(L + 1, 0);
    const double* sg = reinterpret_cast<const double*>(psig);
    for (int q = 0; q < L; ++q) {
        pl->poff[q] = (int)pl->porder.size();
        const size_t at = pl->porder.size();
        for (int t : on[q]) if (t >= nt) pl->porder.push_back(t);
        std::stable_sort(pl->porder.begin() + at, pl->porder.end(), [&](int a, int b) {
            const int ka = pl->K[a], kb = pl->K[b];
            if (ka != kb) return ka < kb;
            const int* ia = pl->rows.data() + pl->ioff[a];
            const int* ib = pl->rows.data() + pl->ioff[b];
            for (int i = 0; i < ka; ++i) if (ia[i] != ib[i]) return ia[i] < ib[i];
            const double* xa = sg + 2 * (size_t)pl->soff[a];
            const double* xb = sg + 2 * (size_t)pl->soff[b];
            for (int i = 0; i < 2 * ka * ka; ++i) if (xa[i] != xb[i]) return xa[i] < xb[i];
            return false;
        });
    }
    pl->poff[L] = (int)pl->porder.size();
    // pair lists: pass 0 takes b on a's layer or a later one, pass 1 b on an earlier one
    pl->pair_at.assign((size_t)2 * L * 3, 0); pl->pair_n.assign((size_t)2 * L * 3, 0);
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < L; ++i) {
            const int p = pass ? L - 1 - i : i;
            std::vector<int> byc[3];
            for (int a : on[p])
                for (int b = 0; b < C; ++b) {
                    const int lb = pl->layer[b];
                    if (pass == 0 ? lb < p : lb >= p) continue;
                    const int cls = tmat_pair_class(pl->K[a], pl->K[b]);
                    byc[cls].push_back(a * C + b);
                    const int ne = pl->K[a] * pl->K[b];
                    pl->max_elems[cls] = std::max(pl->max_elems[cls], ne);
                    if (cls == 0) pl->big_kk = std::max(pl->big_kk, (size_t)ne);
                }
            for (int cls = 0; cls < 3; ++cls) {
                const size_t k = ((size_t)pass * L + i) * 3 + cls;
                pl->pair_at[k] = (int)pl->pairs.size(); pl->pair_n[k] = (int)byc[cls].size();
                pl->pairs.insert(pl->pairs.end(), byc[cls].begin(), byc[cls].end());
            }
        }
    // per energy in flight: two strips of n_max K_tot, the Gamma blocks that depend on E, G_ab | X | Y of the class-0 pairs
    pl->cs = (size_t)ls->nmax * pl->Ktot;
    pl->per_energy = 2 * pl->cs + pl->dyn + 3 * pl->big_kk;
    return NEGF_OK;
}

// the tables, the probes' Sigma and the Gamma blocks that do not depend on E, on the device
int rgf_tmat_setup(negf_ctx* c, LayeredSystem* ls, const cplx* psig, RgfTmatPlan* pl)
{
    std::vector<int> tab;
    size_t at[12]; int k = 0;
    for (const std::vector<int>* v : {&pl->K, &pl->ioff, &pl->goff, &pl->gstride, &pl->soff, &pl->tcol[0], &pl->tcol[1], &pl->rows,
                                      &pl->cpos, &pl->J, &pl->porder, &pl->pairs}) {
        at[k++] = tab.size();
        tab.insert(tab.end(), v->begin(), v->end());
    }
    int rc;
    if ((rc = ensure_cap(c, ls->d_tm_tab, tab.size() + 1)) || (rc = upload(c, ls->d_tm_tab.p, tab.data(), tab.size()))) return rc;
    const int* d = ls->d_tm_tab;
    pl->dK = d + at[0]; pl->d_ioff = d + at[1]; pl->d_goff = d + at[2]; pl->d_gstride = d + at[3]; pl->d_soff = d + at[4];
    pl->d_tcol[0] = d + at[5]; pl->d_tcol[1] = d + at[6]; pl->d_rows = d + at[7]; pl->d_cpos = d + at[8]; pl->d_J = d + at[9];
    pl->d_porder = d + at[10]; pl->d_pairs = d + at[11];
    if ((rc = ensure_cap(c, ls->d_tm_gam, pl->stat + 1))) return rc;
    if (pl->n_probes > 0 && ((rc = ensure_cap(c, ls->d_tm_sig, pl->psum)) || (rc = upload(c, ls->d_tm_sig.p, psig, pl->psum)))) return rc;
    ProfScope ps(c, "tmat");
    launch_tmat_gamma(c->stream, pl->nt, pl->n_probes, 1, pl->dK, pl->d_soff, pl->d_goff, pl->d_gstride, ls->d_tm_sig, 0, ls->d_tm_gam);
    for (int t = 0; t < pl->nt; ++t)
        if (ls->terms[t]->kind == 0) launch_rgf_gamma(c->stream, pl->K[t], 1, ls->terms[t]->d_sig, 0, ls->d_tm_gam + pl->goff[t], 0);
    return NEGF_OK;
}

// the pairs of view level i of a pass, read from the level's strip (n x ld)
void rgf_tmat_pairs(negf_ctx* c, LayeredSystem* ls, const RgfTmatPlan& pl, int pass, int i, int nb, const cplx* strip, int ld, double* T)
{
    const int L = ls->L, C = pl.C, p = pass ? L - 1 - i : i;
    const int col0 = pl.colbase[pass][p];
    const size_t k0 = ((size_t)pass * L + i) * 3;
    if (pl.pair_n[k0] + pl.pair_n[k0 + 1] + pl.pair_n[k0 + 2] == 0) return;
    ProfScope ps(c, "tmat");
    double cmadds = 0;
    for (int cls = 1; cls <= 2; ++cls) {
        launch_rgf_strip_pairs(c->stream, cls, C, pl.pair_n[k0 + cls], pl.max_elems[cls], nb, pl.d_pairs + pl.pair_at[k0 + cls],
                               pl.dK, pl.d_ioff, pl.d_goff, pl.d_gstride, pl.d_tcol[pass], col0, pl.d_rows, pl.d_cpos, strip, ld,
                               pl.cs, ls->d_tm_gam, pl.gdyn, T);
        for (int q = 0; q < pl.pair_n[k0 + cls]; ++q) {
            const int pr = pl.pairs[pl.pair_at[k0 + cls] + q];
            const double ka = pl.K[pr / C], kb = pl.K[pr % C];
            cmadds += ka * kb * (ka + kb);
        }
    }
    negf_count_flops(8.0 * cmadds * nb, 0.0);
    // two lead-sized blocks, or blocks beyond the pair kernel's LDS: gather, two products on the matrix cores, trace
    for (int q = 0; q < pl.pair_n[k0]; ++q) {
        const int pr = pl.pairs[pl.pair_at[k0] + q];
        const int a = pr / C, b = pr - a * C, Ka = pl.K[a], Kb = pl.K[b];
        const size_t kk = (size_t)Ka * Kb;
        const cplx* ga = pl.gstride[a] ? pl.gdyn + pl.goff[a] : ls->d_tm_gam + pl.goff[a];
        const cplx* gb = pl.gstride[b] ? pl.gdyn + pl.goff[b] : ls->d_tm_gam + pl.goff[b];
        launch_gather_block(c->stream, ld, Ka, Kb, nb, strip + (pl.tcol[pass][b] - col0), pl.cs, pl.d_rows + pl.ioff[a],
                            pl.d_cpos + pl.ioff[b], pl.Gab, kk);
        launch_zgemm(c->stream, Ka, Kb, Ka, nb, ga, Ka, (size_t)pl.gstride[a], pl.Gab, Kb, kk, 0, pl.Xs, Kb, kk);
        launch_zgemm(c->stream, Ka, Kb, Kb, nb, pl.Xs, Kb, kk, gb, Kb, (size_t)pl.gstride[b], 0, pl.Ys, Kb, kk);
        launch_trace_dot(c->stream, Ka, Kb, nb, pl.Ys, Kb, kk, pl.Gab, Kb, kk, T + (size_t)a * C + b, C * C);
    }
}

// One pass of the batch [m0, m0 + nb): forward sweep with the g_i kept (the probes in the diagonal), backward sweep with
// the column strips, the pairs of every level consumed from its strip.  Level i of the view is layer p(i) = i (pass 0) or
// L - 1 - i (pass 1); the view's C_{i,i+1} is the lower block of the pair in pass 1.  Work areas: buf[0..8], d_gstore.
int rgf_tmat_pass(negf_ctx* c, const RgfRun& r, const RgfTmatPlan& pl, int pass, int m0, int nb, const cplx* E, double* T)
{
    LayeredSystem* ls = r.ls;
    const int L = ls->L;
    const size_t s = ls->stride;
    const size_t layer_bytes = (size_t)nb * s * sizeof(cplx);
    cplx *CU = r.buf[0], *CL = r.buf[1], *U = r.buf[2], *V = r.buf[3], *Wm = r.buf[4], *Gup = r.buf[5], *B = r.buf[6];
    cplx *Gcur = r.buf[7], *Galt = r.buf[8];
    int* info = c->d_info + m0;
    auto phys = [&](int i) { return pass ? L - 1 - i : i; };
    auto g_of = [&](int i) { return ls->d_gstore + (size_t)i * r.nb_max * s; };
    // the negated couplings between view levels i and i + 1: CU = C_{i,i+1}, CL = C_{i+1,i}
    auto couplings = [&](int i) {
        ProfScope ps(c, "rgf");
        const int q = pass ? phys(i + 1) : i;                          // the pair (q, q + 1) of the system
        const int cnt = ls->n[q] * ls->n[q + 1];
        const cplx *Su = ls->dSu + ls->uoff[q], *Fu = ls->dFu + ls->uoff[q], *Sl = ls->dSl + ls->uoff[q], *Fl = ls->dFl + ls->uoff[q];
        launch_rgf_coupling(c->stream, cnt, nb, E + m0, pass ? Sl : Su, pass ? Fl : Fu, CU, s);
        launch_rgf_coupling(c->stream, cnt, nb, E + m0, pass ? Su : Sl, pass ? Fu : Fl, CL, s);
    };
    int rc;
    for (int i = 0; i < L; ++i) {
        const int p = phys(i), ni = ls->n[p];
        cplx* D = g_of(i);
        if (i > 0) {
            const int np = ls->n[phys(i - 1)];
            couplings(i - 1);
            rgf_mm(c, ls, ni, np, np, nb, CL, g_of(i - 1), U);         // C_{i,i-1} g_{i-1}
            rgf_mm(c, ls, ni, ni, np, nb, U, CU, V);                   // ... C_{i-1,i}
        }
        rgf_assemble_diag(c, ls, p, m0, nb, E, i > 0 ? V : nullptr, D);
        if (pl.poff[p + 1] > pl.poff[p]) {
            ProfScope ps(c, "rgf");
            launch_rgf_sub_probes(c->stream, ni, pl.poff[p + 1] - pl.poff[p], nb, pl.d_porder + pl.poff[p], pl.dK, pl.d_ioff,
                                  pl.d_soff, pl.d_rows, ls->d_tm_sig, D, s);
        }
        cplx* g = nullptr;
        if ((rc = rgf_inverse(c, ls, p, nb, D, B, info, &g))) return rc;
        if (g != D) NEGF_HIP_CHECK(hipMemcpyAsync(D, g, layer_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    cplx *Scur = pl.strip[0], *Snext = pl.strip[1];
    const cplx* Gnext = g_of(L - 1);
    int wnext = 0;                                                     // width of the strip of level i + 1
    for (int i = L - 1; i >= 0; --i) {
        const int p = phys(i), ni = ls->n[p], nj = pl.nJ[p], w = nj + wnext;
        const cplx* Gii = Gnext;
        if (i < L - 1) {
            const int nn = ls->n[phys(i + 1)];
            const cplx* g = g_of(i);
            couplings(i);
            rgf_mm(c, ls, ni, nn, ni, nb, g, CU, U);                   // U = g_i C_{i,i+1}
            rgf_mm(c, ls, ni, nn, nn, nb, U, Gnext, Gup);              // G_{i,i+1}
            rgf_mm(c, ls, nn, ni, ni, nb, CL, g, V);                   // V = C_{i+1,i} g_i
            rgf_mm(c, ls, ni, ni, nn, nb, Gup, V, Wm);
            { ProfScope ps(c, "rgf"); launch_rgf_add(c->stream, ni * ni, nb, g, s, Wm, s, Gcur, s); }
            Gii = Gcur;
            if (wnext > 0) {
                ProfScope ps(c, "zgemm");                              // U_i strip_{i+1} behind the head of strip_i
                launch_zgemm(c->stream, ni, wnext, nn, nb, U, nn, s, Snext, wnext, pl.cs, 0, Scur + nj, w, pl.cs);
            }
        }
        if (nj > 0) {
            ProfScope ps(c, "rgf");
            launch_rgf_strip_head(c->stream, ni, nj, w, nb, Gii, s, pl.d_J + pl.Joff[p], Scur, pl.cs);
        }
        rgf_tmat_pairs(c, ls, pl, pass, i, nb, Scur, w, T);
        if (i < L - 1) { Gnext = Gcur; std::swap(Gcur, Galt); }
        std::swap(Scur, Snext);
        wnext = w;
    }
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

}  // namespace

extern "C" {

int negf_layered_create(negf_ctx* c, int n_layers, const int* sizes, const double* F_diag, const double* F_up,
                        const double* S_diag, const double* S_up, int* handle)
{
    if (!c || !sizes || !F_diag || !F_up || !S_diag || !S_up || !handle) return NEGF_EINVAL;
    if (n_layers < 2) return NEGF_EINVAL;
    long long N = 0;
    for (int i = 0; i < n_layers; ++i) {
        if (sizes[i] < 1 || sizes[i] > 8192) return NEGF_EINVAL;        // what the inverse kernels serve
        N += sizes[i];
    }
    if (N > (1LL << 30)) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    LayeredSystem* ls = new LayeredSystem();
    ls->L = n_layers; ls->N = (int)N;
    ls->n.assign(sizes, sizes + n_layers);
    ls->off.resize(n_layers); ls->doff.resize(n_layers); ls->uoff.resize(n_layers - 1);
    for (int i = 0, o = 0; i < n_layers; ++i) {
        ls->off[i] = o; o += sizes[i];
        ls->doff[i] = ls->dtot; ls->dtot += (size_t)sizes[i] * sizes[i];
        if (i + 1 < n_layers) { ls->uoff[i] = ls->utot; ls->utot += (size_t)sizes[i] * sizes[i + 1]; }
        ls->nmax = std::max(ls->nmax, sizes[i]);
    }
    ls->stride = (size_t)ls->nmax * ls->nmax;
    // the lower blocks are the conjugate transposes of the upper ones: formed once on the host, so that every
    // per-energy pass reads its block row-major
    const cplx* Fu = reinterpret_cast<const cplx*>(F_up);
    const cplx* Su = reinterpret_cast<const cplx*>(S_up);
    std::vector<cplx> Fl(ls->utot), Sl(ls->utot);
    for (int i = 0; i + 1 < n_layers; ++i) {
        const int a = sizes[i], b = sizes[i + 1];
        const size_t o = ls->uoff[i];
        for (int r = 0; r < b; ++r)
            for (int q = 0; q < a; ++q) {
                Fl[o + (size_t)r * a + q] = cconj(Fu[o + (size_t)q * b + r]);
                Sl[o + (size_t)r * a + q] = cconj(Su[o + (size_t)q * b + r]);
            }
    }
    int rc;
    if ((rc = dev_alloc(&ls->dFd, ls->dtot)) || (rc = dev_alloc(&ls->dSd, ls->dtot)) ||
        (rc = dev_alloc(&ls->dFu, ls->utot)) || (rc = dev_alloc(&ls->dSu, ls->utot)) ||
        (rc = dev_alloc(&ls->dFl, ls->utot)) || (rc = dev_alloc(&ls->dSl, ls->utot)) ||
        (rc = upload(c, ls->dFd, reinterpret_cast<const cplx*>(F_diag), ls->dtot)) ||
        (rc = upload(c, ls->dSd, reinterpret_cast<const cplx*>(S_diag), ls->dtot)) ||
        (rc = upload(c, ls->dFu, Fu, ls->utot)) || (rc = upload(c, ls->dSu, Su, ls->utot)) ||
        (rc = upload(c, ls->dFl, Fl.data(), ls->utot)) || (rc = upload(c, ls->dSl, Sl.data(), ls->utot))) { free_layered(ls); return rc; }
    c->layered.push_back(ls);
    *handle = (int)c->layered.size() - 1;
    return NEGF_OK;
}

int negf_layered_free(negf_ctx* c, int h)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls) return NEGF_EINVAL;
    (void)hipStreamSynchronize(c->stream);
    free_layered(ls);
    c->layered[h] = nullptr;
    return NEGF_OK;
}

int negf_layered_terminal_const(negf_ctx* c, int h, int layer, int K, const int* inds, const double* sigma, int* terminal)
{
    if (!sigma) return NEGF_EINVAL;
    LayeredSystem* ls; RgfTerminal* t;
    int rc = rgf_new_terminal(c, h, layer, K, inds, terminal, &ls, &t);
    if (rc) return rc;
    t->kind = 0;
    const size_t kk = (size_t)K * K;
    if ((rc = dev_alloc(&t->d_sig, kk)) || (rc = upload(c, t->d_sig, reinterpret_cast<const cplx*>(sigma), kk))) { free_terminal(t); return rc; }
    *terminal = rgf_add_terminal(ls, t);
    return NEGF_OK;
}

int negf_layered_terminal_blocks(negf_ctx* c, int h, int layer, int K, const int* inds, int m, const double* sigma, int* terminal)
{
    if (!sigma || m < 1) return NEGF_EINVAL;
    LayeredSystem* ls; RgfTerminal* t;
    int rc = rgf_new_terminal(c, h, layer, K, inds, terminal, &ls, &t);
    if (rc) return rc;
    t->kind = 2; t->m_blk = m;
    const size_t cnt = (size_t)K * K * m;
    if ((rc = dev_alloc(&t->d_sig, cnt)) || (rc = upload(c, t->d_sig, reinterpret_cast<const cplx*>(sigma), cnt))) { free_terminal(t); return rc; }
    *terminal = rgf_add_terminal(ls, t);
    return NEGF_OK;
}

int negf_layered_terminal_chain(negf_ctx* c, int h, int layer, int K, const int* inds,
                                const double* alpha, const double* Salpha, const double* beta, const double* Sbeta,
                                const double* tau, const double* Stau, double eta, double conv, double relFactor,
                                int max_iter, int force_iters, int solver, int* terminal)
{
    if (solver != 0 && solver != 1) return NEGF_EINVAL;
    if (solver == 1 && (!(conv >= 0.0) || max_iter < 0)) return NEGF_EINVAL;
    LayeredSystem* ls; RgfTerminal* t;
    int rc = rgf_new_terminal(c, h, layer, K, inds, terminal, &ls, &t);
    if (rc) return rc;
    t->kind = 1;
    // one CHAIN1D provider with one contact, its index list inside the layer: the chain kernels, the job order and the
    // g(E) cache serve it as they serve a dense system's lead
    if ((rc = make_chain1d(c, ls->n[layer], 1, &K, inds, alpha, Salpha, beta, Sbeta, tau, Stau, eta, conv,
                           solver == 1 ? 1.0 : relFactor, max_iter, force_iters, &t->chain))) { free_terminal(t); return rc; }
    t->chain->solver = solver;
    *terminal = rgf_add_terminal(ls, t);
    return NEGF_OK;
}

int negf_layered_terminal_sigma(negf_ctx* c, int h, int terminal, int m, const double* E, double* sigma_out)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (terminal < 0 || terminal >= (int)ls->terms.size() || (m > 0 && (!E || !sigma_out))) return NEGF_EINVAL;
    RgfTerminal* t = ls->terms[terminal];
    const size_t kk = (size_t)t->K * t->K;
    cplx* out = reinterpret_cast<cplx*>(sigma_out);
    if (t->kind == 0) { for (int b = 0; b < m; ++b) if ((rc = download(c, out + kk * b, t->d_sig, kk))) return rc; return NEGF_OK; }
    if (t->kind == 2) return download(c, out, t->d_sig, kk * m);
    if ((rc = stage_grid(c, m, 1, E, nullptr))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, false, &r))) return rc;
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        if ((rc = run_sigma_blocks(c, t->chain, nb, c->d_E + m0, ls->d_iters, ls->d_conv, m0, t->d_blk.p))) return rc;
        if ((rc = download(c, out + kk * m0, t->d_blk.p, kk * nb))) return rc;
    }
    return NEGF_OK;
}

int negf_layered_transmission_dev(negf_ctx* c, int h, int term_a, int term_b, int m, const double* E_dev, double* T_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    const int nt = (int)ls->terms.size();
    if (term_a < 0 || term_a >= nt || term_b < 0 || term_b >= nt) return NEGF_EINVAL;
    RgfTerminal *ta = ls->terms[term_a], *tb = ls->terms[term_b];
    if (ta->end == tb->end) return NEGF_EINVAL;                     // the corner blocks connect opposite end layers only
    if (!T_dev || (m > 0 && !E_dev)) return NEGF_EINVAL;
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, false, &r))) return rc;
    const int Ka = ta->K, Kb = tb->K;
    const size_t kab = (size_t)Ka * Kb, sa = (size_t)Ka * Ka, sb = (size_t)Kb * Kb;
    const size_t per = sa + sb + 3 * kab;
    if ((rc = ensure_cap(c, ls->d_small, per * r.nb_max))) return rc;
    cplx* gamA = ls->d_small;
    cplx* gamB = gamA + sa * r.nb_max;
    cplx* Gab = gamB + sb * r.nb_max;
    cplx* Xs = Gab + kab * r.nb_max;
    cplx* Ys = Xs + kab * r.nb_max;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    // a on the last layer: G_ab is cut from G_{L-1,0} (X); a on layer 0: from G_{0,L-1} (Y)
    const int corner = ta->end == 1 ? 1 : 2;
    const int ld = corner == 1 ? ls->n[0] : ls->n[ls->L - 1];
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        cplx* Gc = nullptr;
        if ((rc = rgf_forward(c, r, m0, nb, E, false, corner, &Gc))) return rc;
        const cplx *sA, *sB; size_t stA, stB;
        rgf_sigma_of(ta, m0, &sA, &stA); rgf_sigma_of(tb, m0, &sB, &stB);
        {
            ProfScope ps(c, "gamma");
            launch_rgf_gamma(c->stream, Ka, nb, sA, stA, gamA, sa);
            launch_rgf_gamma(c->stream, Kb, nb, sB, stB, gamB, sb);
        }
        {
            ProfScope ps(c, "zgemm");
            launch_gather_block(c->stream, ld, Ka, Kb, nb, Gc, ls->stride, ta->d_idx, tb->d_idx, Gab, kab);
            launch_zgemm(c->stream, Ka, Kb, Ka, nb, gamA, Ka, sa, Gab, Kb, kab, 0, Xs, Kb, kab);
            launch_zgemm(c->stream, Ka, Kb, Kb, nb, Xs, Kb, kab, gamB, Kb, sb, 0, Ys, Kb, kab);
        }
        ProfScope ps(c, "trace");
        launch_trace_dot(c->stream, Ka, Kb, nb, Ys, Kb, kab, Gab, Kb, kab, T_dev + m0, 1);
    }
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_transmission(negf_ctx* c, int h, int term_a, int term_b, int m, const double* E, double* T, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (m > 0 && (!E || !T)) return NEGF_EINVAL;
    const int nt = (int)ls->terms.size();
    if (term_a < 0 || term_a >= nt || term_b < 0 || term_b >= nt || ls->terms[term_a]->end == ls->terms[term_b]->end) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    if ((rc = stage_grid(c, m, 1, E, nullptr, (size_t)m * sizeof(double)))) return rc;
    if ((rc = negf_layered_transmission_dev(c, h, term_a, term_b, m, reinterpret_cast<double*>(c->d_E), c->d_scal))) return rc;
    return fetch_result_and_info(c, m, c->d_scal, (size_t)m * sizeof(double), T, info);
}

int negf_layered_dos_dev(negf_ctx* c, int h, int form, int m, const double* E_dev, double* dos_total_dev, double* dos_site_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if ((form != 0 && form != 1) || (m > 0 && (!E_dev || !dos_total_dev || !dos_site_dev))) return NEGF_EINVAL;
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, true, &r))) return rc;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    RgfDosArg arg{form, dos_site_dev};
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        if ((rc = rgf_forward(c, r, m0, nb, E, true, 0, nullptr))) return rc;
        if ((rc = rgf_backward(c, r, m0, nb, E, rgf_consume_dos, &arg))) return rc;
        ProfScope ps(c, "rgf");
        launch_rgf_dos_total(c->stream, ls->N, nb, dos_site_dev + (size_t)m0 * ls->N, (size_t)ls->N, dos_total_dev + m0);
    }
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_dos(negf_ctx* c, int h, int form, int m, const double* E, double* dos_total, double* dos_site, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if ((form != 0 && form != 1) || (m > 0 && (!E || !dos_total))) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    if ((rc = stage_grid(c, m, 1, E, nullptr))) return rc;
    if ((rc = ensure_cap(c, ls->d_site, (size_t)m * ls->N))) return rc;
    if ((rc = negf_layered_dos_dev(c, h, form, m, reinterpret_cast<double*>(c->d_E), c->d_scal, ls->d_site))) return rc;
    if (dos_site && (rc = download(c, dos_site, ls->d_site.p, (size_t)m * ls->N))) return rc;
    if ((rc = download(c, dos_total, c->d_scal, (size_t)m))) return rc;
    return reduce_info(c, m, info);
}

int negf_layered_gr_int_dev(negf_ctx* c, int h, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, true, &r))) return rc;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    RgfSumArg arg{reinterpret_cast<const cplx*>(w_dev), reinterpret_cast<cplx*>(out_dev)};
    NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, (ls->dtot + 2 * ls->utot) * sizeof(cplx), c->stream));
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        if ((rc = rgf_forward(c, r, m0, nb, E, true, 0, nullptr))) return rc;
        if ((rc = rgf_backward(c, r, m0, nb, E, rgf_consume_sum, &arg))) return rc;
    }
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_gr_int(negf_ctx* c, int h, int m, const double* E, const double* w, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    const size_t tot = ls->dtot + 2 * ls->utot;
    if ((rc = stage_grid(c, m, 1, E, w, tot * sizeof(cplx)))) return rc;
    if ((rc = ensure_cap(c, ls->d_out, tot))) return rc;
    if ((rc = negf_layered_gr_int_dev(c, h, m, reinterpret_cast<double*>(c->d_E), reinterpret_cast<double*>(c->d_w),
                                      reinterpret_cast<double*>(ls->d_out.p)))) return rc;
    return fetch_result_and_info(c, m, ls->d_out.p, tot * sizeof(cplx), out, info);
}

int negf_layered_gless_int_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    RgfLess less;
    if ((rc = rgf_less_select(c, ls, ind, &less))) return rc;
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, true, &r, less.per_energy))) return rc;
    rgf_less_layout(r, &less);
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    RgfSumArg arg{reinterpret_cast<const cplx*>(w_dev), reinterpret_cast<cplx*>(out_dev)};
    less.consume = rgf_consume_less_sum; less.arg = &arg;
    NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, (ls->dtot + 2 * ls->utot) * sizeof(cplx), c->stream));
    for (int m0 = 0; m0 < m; m0 += r.nb_max)
        if ((rc = rgf_less_batch(c, r, &less, m0, std::min(r.nb_max, m - m0), E))) return rc;
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_gless_int(negf_ctx* c, int h, int ind, int m, const double* E, const double* w, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    if (!rgf_less_ind_ok(ls, ind)) return NEGF_EINVAL;
    const size_t tot = ls->dtot + 2 * ls->utot;
    if ((rc = stage_grid(c, m, 1, E, w, tot * sizeof(cplx)))) return rc;
    if ((rc = ensure_cap(c, ls->d_out, tot))) return rc;
    if ((rc = negf_layered_gless_int_dev(c, h, ind, m, reinterpret_cast<double*>(c->d_E), reinterpret_cast<double*>(c->d_w),
                                         reinterpret_cast<double*>(ls->d_out.p)))) return rc;
    return fetch_result_and_info(c, m, ls->d_out.p, tot * sizeof(cplx), out, info);
}

int negf_layered_contact_dos_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, double* dos_total_dev, double* dos_site_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (m > 0 && (!E_dev || !dos_total_dev || !dos_site_dev)) return NEGF_EINVAL;
    RgfLess less;
    if ((rc = rgf_less_select(c, ls, ind, &less))) return rc;
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, true, &r, less.per_energy))) return rc;
    rgf_less_layout(r, &less);
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    less.consume = rgf_consume_less_dos; less.arg = dos_site_dev;
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        if ((rc = rgf_less_batch(c, r, &less, m0, nb, E))) return rc;
        ProfScope ps(c, "rgf");
        launch_rgf_dos_total(c->stream, ls->N, nb, dos_site_dev + (size_t)m0 * ls->N, (size_t)ls->N, dos_total_dev + m0);
    }
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_contact_dos(negf_ctx* c, int h, int ind, int m, const double* E, double* dos_total, double* dos_site, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (m > 0 && (!E || !dos_total)) return NEGF_EINVAL;
    if (!rgf_less_ind_ok(ls, ind)) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    if ((rc = stage_grid(c, m, 1, E, nullptr))) return rc;
    if ((rc = ensure_cap(c, ls->d_site, (size_t)m * ls->N))) return rc;
    if ((rc = negf_layered_contact_dos_dev(c, h, ind, m, reinterpret_cast<double*>(c->d_E), c->d_scal, ls->d_site))) return rc;
    if (dos_site && (rc = download(c, dos_site, ls->d_site.p, (size_t)m * ls->N))) return rc;
    if ((rc = download(c, dos_total, c->d_scal, (size_t)m))) return rc;
    return reduce_info(c, m, info);
}

int negf_layered_transmission_matrix_dev(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                         const double* probe_sigma, int m, const double* E_dev, double* T_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    RgfTmatPlan pl;
    const cplx* psig = reinterpret_cast<const cplx*>(probe_sigma);
    if ((rc = rgf_tmat_plan(ls, n_probes, probe_nk, probe_inds, psig, &pl))) return rc;
    if (m > 0 && (!E_dev || !T_dev)) return NEGF_EINVAL;
    if (m == 0) { c->last_m = 0; return NEGF_OK; }
    if ((rc = ensure_mbuffers(c, m, 1))) return rc;
    RgfRun r;
    if ((rc = rgf_workspace(c, ls, m, true, &r, pl.per_energy))) return rc;
    ls->work_bytes += 16LL * (long long)pl.stat;
    if ((rc = rgf_tmat_setup(c, ls, psig, &pl))) return rc;
    {
        const size_t nbm = (size_t)r.nb_max;
        cplx* q = ls->d_cols.p;
        pl.strip[0] = q; q += pl.cs * nbm;
        pl.strip[1] = q; q += pl.cs * nbm;
        pl.gdyn = q; q += pl.dyn * nbm;
        pl.Gab = q; q += pl.big_kk * nbm;
        pl.Xs = q; q += pl.big_kk * nbm;
        pl.Ys = q;
    }
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    const size_t C2 = (size_t)pl.C * pl.C;
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const int nb = std::min(r.nb_max, m - m0);
        double* T = T_dev + C2 * m0;
        NEGF_HIP_CHECK(hipMemsetAsync(c->d_info + m0, 0, (size_t)nb * sizeof(int), c->stream));
        if ((rc = rgf_chain_sigmas(c, ls, m0, nb, E))) return rc;
        {
            ProfScope ps(c, "tmat");
            for (int t = 0; t < pl.nt; ++t) {
                if (ls->terms[t]->kind == 0) continue;
                const cplx* sig; size_t st;
                rgf_sigma_of(ls->terms[t], m0, &sig, &st);
                launch_rgf_gamma(c->stream, pl.K[t], nb, sig, st, pl.gdyn + pl.goff[t], pl.dyn);
            }
        }
        for (int pass = 0; pass < (pl.two_pass ? 2 : 1); ++pass)
            if ((rc = rgf_tmat_pass(c, r, pl, pass, m0, nb, E, T))) return rc;
        ProfScope ps(c, "tmat");
        launch_tmat_nan(c->stream, pl.C, nb, c->d_info + m0, T);
    }
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

int negf_layered_transmission_matrix(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                     const double* probe_sigma, int m, const double* E, double* T, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    const long Cl = (long)ls->terms.size() + n_probes;
    if (n_probes < 0 || Cl < 1 || Cl > TMAT_MAX_TERMINALS || (m > 0 && (!E || !T))) return NEGF_EINVAL;
    if ((rc = stage_grid(c, m, 1, E, nullptr))) return rc;
    const size_t C = ls->terms.size() + (size_t)n_probes, cnt = (size_t)m * C * C;
    if ((rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_layered_transmission_matrix_dev(c, h, n_probes, probe_nk, probe_inds, probe_sigma, m,
                                                   reinterpret_cast<double*>(c->d_E), c->d_bond_T))) return rc;
    if ((rc = download(c, T, c->d_bond_T.p, cnt))) return rc;
    return reduce_info(c, m, info);
}

int negf_layered_workspace_bytes(negf_ctx* c, int h, long long* work)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls || !work) return NEGF_EINVAL;
    *work = ls->work_bytes;
    return NEGF_OK;
}

}  // extern "C"
