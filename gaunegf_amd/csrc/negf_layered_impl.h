// Recursive Green's function path for layered (block-tridiagonal) devices: the negf_layered_* entry points of
// include/negf.h and the eigenchannel entry points of include/negf_layered_channels.h.  Part of negf_api.hip's translation unit (included at its end): it uses that file's allocation,
// staging and self-energy helpers as they are.
//
// A LayeredSystem is an object of its own inside the context: blocks, terminals and workspace are its own, the dense
// system (negf_set_system), its providers and its workspace are never read or written here.  What is shared is
// per-call staging with no meaning between calls: the grid / info / scalar buffers (ensure_mbuffers), the pinned host
// buffer, the Sigma kernels' scratch and the g(E) cache of the chain leads.
//
// Per energy, with C_ij = F_ij - E S_ij (the NEGATED coupling -A_ij: every sign of the textbook recursion cancels):
//   factor     g_0 = (A_00 - Sigma_left)^-1,   g_i = (A_ii - C_{i,i-1} g_{i-1} C_{i-1,i} - [i = L-1] Sigma_right)^-1
//   corner     X_0 = g_0,  X_i = g_i C_{i,i-1} X_{i-1}  -> G_{L-1,0};    Y_i = Y_{i-1} C_{i-1,i} g_i  -> G_{0,L-1}
//   solve      G_{L-1,L-1} = g_{L-1};  U = g_i C_{i,i+1},  V = C_{i+1,i} g_i:
//              G_{i,i+1} = U G_{i+1,i+1},   G_{i+1,i} = G_{i+1,i+1} V,   G_ii = g_i + G_{i,i+1} V
//   columns    of a terminal set on the union J of its orbitals (G Gamma G^H on the pattern of S), W_i = G_{i,end}[:, J]:
//              last layer:  W_{L-1} = G_{L-1,L-1}[:, J],  W_i = U_i W_{i+1}                    (solve sweep)
//              layer 0:     x_0 = g_0[:, J],  z_i = C_{i,i-1} x_{i-1},  x_i = g_i z_i          (factor sweep, the z_i kept)
//                           W_0 = G_00[:, J],  W_i = G_ii z_i                                  (solve sweep)
//              A_ii = (W_i Gamma) W_i^H,   A_{i,i+1} = (W_i Gamma) W_{i+1}^H,   A_{i+1,i} = A_{i,i+1}^H never formed
//   strips     of the transmission matrix between ALL terminals, probes on any layer included (rgf_tmat_*): with J_q the
//              union of the orbitals of the terminals on layer q,
//              strip_{L-1} = [G_{L-1,L-1}[:, J_{L-1}]],   strip_i = [G_ii[:, J_i] | U_i strip_{i+1}]   (solve sweep)
//              holds G_{i,q}[:, J_q] for every q >= i: the pairs (a on layer i, b on a layer >= i) are read from it, the
//              pairs with b on an earlier layer from the same pass over the layers in REVERSE order
// Every layer matrix of a batch is compact row-major at ONE batch stride (the largest layer's n^2): the inverses and
// products are the dense path's launchers, batched over the energies.
//
// The recursion stands once.  rgf_factor_sweep keeps every g_i in d_gstore and takes two callables, run before and after
// the inverse of a level (the strips' probes; the columns' x / z chain); rgf_solve_sweep hands each level as it stands
// (RgfLevel) to a visitor: the block visitors RgfSumBlocks / RgfDosBlocks / RgfBondBlocks (the last one behind the
// column visitor only), the column visitor RgfColumns, the strip visitors RgfStrips (two alternating strips) and RgfKeptStrips
// (the strips of all layers kept, for the floating-probe calls), which share rgf_strip_level.  Only a block visitor has G_{i+1,i} formed.  rgf_corner_sweep shares the level (rgf_factor_level) but
// not the loop: it alone lets g_{i-2} go.  All of them walk the levels of an RgfView, which the strips' second pass reverses.
// The ten work areas have names (RgfAreas says who writes each, and when); the two places that lend one out say so:
// rgf_corner_sweep and RgfColumns::level.  Every device-resident call is its checks, its work areas, then rgf_batches.

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
    DevBuf<cplx> d_chan;                        // eigenchannels: Gamma_a | Gamma_b | G_ab | Z | W | H | the wide solver's copy of H
                                                // per energy in flight, then L^H (once for a const terminal)
    DevBuf<int> d_chan_rank;                    // ... the rank of every L^H
    DevBuf<double> d_chan_T;                    // ... [m][nchan] staging of the host-pointer entry point
    DevBuf<cplx> d_cols;                        // column sets of G Gamma G^H: z_i | x | W | Y | Gamma, per energy in flight;
                                                // of a transmission matrix: strip | strip | Gamma(E) | G_ab | X | Y
    DevBuf<int> d_J;                            // [2][nmax] their union lists, layer 0's then the last layer's
    DevBuf<cplx> d_out;                         // gr_int: the block lists, host-pointer entry point
    DevBuf<double> d_site;                      // dos: [m][N] staging of the host-pointer entry point
    DevBuf<int> d_tm_tab;                       // transmission matrix: the terminal tables, union lists and pair lists
    DevBuf<cplx> d_tm_sig, d_tm_gam;            // ... the probes' Sigma blocks; the Gamma blocks that do not depend on E
    DevBuf<int> d_deph_tab;                     // floating probes: the tables of the coupling and block-diagonal kernels
    DevBuf<double> d_deph_T, d_deph_R;          // ... [batch][C*C] matrices and [batch][P][n_t] responses of the batch in flight
    DevBuf<double> d_deph_out;                  // ... [m][P][n_t] staging of the host-pointer response
    DevBuf<int> d_bond_map;                     // bond tables: perm [N] (layer by layer) | goff [sum (g_i + 1)] of the call's groups
    DevBuf<double> d_bond_out;                  // ... the staging of the host-pointer entry points
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
    release_bufs(ls->d_site, ls->d_chan_T);
    release_bufs(ls->d_chan);
    release_bufs(ls->d_chan_rank);
    release_bufs(ls->d_J, ls->d_tm_tab, ls->d_bond_map);
    release_bufs(ls->d_bond_out);
    release_bufs(ls->d_tm_sig, ls->d_tm_gam);
    release_bufs(ls->d_deph_tab);
    release_bufs(ls->d_deph_T, ls->d_deph_R, ls->d_deph_out);
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
struct RgfLess {
    int K[2] = {0, 0};                          // |J|, 0: no terminal of that end selected
    const int* J[2] = {nullptr, nullptr};       // device, ascending
    const RgfTerminal* only = nullptr;          // the one terminal selected, null: all
    size_t cs = 0, per_energy = 0;
    cplx *z = nullptr, *x[2] = {nullptr, nullptr};          // layer-0 set: z_1 .. z_{L-1} [L-1][batch][cs], x_{i-1} | x_i
    cplx *W[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *Y[2] = {nullptr, nullptr}, *gam[2] = {nullptr, nullptr};
};

// The RGF_NBUF work areas of a sweep, each [batch][stride], in the order they lie in the pool.  A factor sweep is over
// before the solve sweep of the same batch starts, so the two name their own uses of one area.
struct RgfAreas {
    cplx *CU, *CL;              // the negated couplings of the level pair at hand
    cplx *U, *V;                // solve: g_i C_{i,i+1}, C_{i+1,i} g_i;  factor: C_{i,i-1} g_{i-1}, then the Schur term
    cplx *W;                    // solve: G_{i,i+1} V
    cplx *Gup, *Glo;            // solve: G_{i,i+1}, G_{i+1,i};  factor: Glo is the inverse's second area
    cplx* Gii[2];               // solve: G_ii of this level and of the level before it, alternating
    cplx* spare;                // nobody's: a visitor may use it
};

struct RgfRun {
    negf_ctx* c;
    LayeredSystem* ls;
    int nb_max;                 // energies per sweep
    RgfAreas a;
    cplx* g(int i) const { return ls->d_gstore + (size_t)i * nb_max * ls->stride; }     // the kept g of level i
};

// one batch [m0, m0 + nb) of a run on its way through the sweeps; E: the whole grid, on the device
struct RgfBatch : RgfRun {
    int m0, nb;
    const cplx* E;
};

// hands out consecutive areas of a buffer that holds a call's small per-batch areas
struct RgfCarve {
    cplx* p;
    cplx* take(size_t count) { cplx* q = p; p += count; return q; }
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
    r->c = c; r->ls = ls; r->nb_max = want;
    RgfCarve pool{ls->d_pool.p};
    RgfAreas& a = r->a;
    for (cplx** area : {&a.CU, &a.CL, &a.U, &a.V, &a.W, &a.Gup, &a.Glo, &a.Gii[0], &a.Gii[1], &a.spare}) *area = pool.take((size_t)want * s);
    static_assert(sizeof(RgfAreas) == RGF_NBUF * sizeof(cplx*), "RGF_NBUF areas");
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
void rgf_assemble_diag(const RgfBatch& b, int i, const cplx* P, cplx* D)
{
    ProfScope ps(b.c, "rgf");
    const LayeredSystem* ls = b.ls;
    const RgfTermArgs ta = rgf_term_args(ls, i == 0 ? 0 : i == ls->L - 1 ? 1 : -1, b.m0);
    launch_rgf_diag(b.c->stream, ls->n[i], b.nb, b.E + b.m0, ls->dSd + ls->doff[i], ls->dFd + ls->doff[i], P, ls->stride, ta, D, ls->stride);
}

// The layers in the order a sweep visits them: level i is layer i, or layer L - 1 - i when reversed -- a view, no block
// is copied.  The sweeps speak of levels only.
struct RgfView {
    const LayeredSystem* ls;
    bool reversed;
    int layer(int i) const { return reversed ? ls->L - 1 - i : i; }
    int n(int i) const { return ls->n[layer(i)]; }
    // the negated couplings of the levels (i, i+1): CU = C_{i,i+1} (n_i x n_{i+1}), CL = C_{i+1,i}; reversed, the
    // upper block of the pair of layers is the view's lower one
    void couplings(const RgfBatch& b, int i) const
    {
        ProfScope ps(b.c, "rgf");
        const int q = std::min(layer(i), layer(i + 1));                  // the pair (q, q + 1) of the system
        const int cnt = ls->n[q] * ls->n[q + 1];
        const cplx *Su = ls->dSu + ls->uoff[q], *Fu = ls->dFu + ls->uoff[q], *Sl = ls->dSl + ls->uoff[q], *Fl = ls->dFl + ls->uoff[q];
        launch_rgf_coupling(b.c->stream, cnt, b.nb, b.E + b.m0, reversed ? Sl : Su, reversed ? Fl : Fu, b.a.CU, ls->stride);
        launch_rgf_coupling(b.c->stream, cnt, b.nb, b.E + b.m0, reversed ? Su : Sl, reversed ? Fu : Fl, b.a.CL, ls->stride);
    }
};

// C[b] (M x N) = A[b] (M x K) B[b] (K x N), all compact at the system's stride
void rgf_mm(const RgfBatch& b, int M, int N, int K, const cplx* A, const cplx* B, cplx* C)
{
    ProfScope ps(b.c, "zgemm");
    const size_t s = b.ls->stride;
    launch_zgemm(b.c->stream, M, N, K, b.nb, A, K, s, B, N, s, 0, C, N, s);
}

// In-place inverse of the n x n matrices in A with B as the blocked kernels' second area: *res = where the inverses
// lie.  A zero pivot of layer i is reported as column off_i + k of the whole system.
int rgf_inverse(const RgfBatch& b, int i, cplx* A, cplx* B, cplx** res)
{
    negf_ctx* c = b.c;
    LayeredSystem* ls = b.ls;
    const int n = ls->n[i], nb = b.nb;
    {
        ProfScope ps(c, "inverse");
        int algo = c->inverse_algo;
        c->gj_last = GjRecord{};
        c->gj_last.path = 0;
        if (algo == 0) algo = inverse_blocked_supported(n) ? 2 : 1;
        const int win_mode = algo == 3 ? 1 : algo == 4 ? 2 : 0;
        if (algo > 2) algo = 2;
        bool in_b = false;
        if (algo == 2) {
            in_b = launch_inverse_blocked(c->stream, n, nb, A, B, ls->stride, ls->d_piv, ls->d_linfo, &c->gj_side, win_mode, nullptr, &c->gj_last);
            if (!in_b) algo = 1;
        }
        if (algo == 1 && !launch_inverse_unblocked(c->stream, n, nb, A, ls->d_linfo, ls->stride)) return NEGF_EINVAL;
        NEGF_HIP_CHECK(hipGetLastError());
        const double dn = n, np = (double)((n + 15) & ~15), k4 = (double)((n + 3) & ~3);
        negf_count_flops(8.0 * dn * dn * dn * nb, algo == 2 ? 6.0 * np * np * k4 * nb - inverse_blocked_vector_flops() : 0.0);
        *res = in_b ? B : A;
    }
    launch_rgf_merge_info(c->stream, nb, ls->off[i], ls->d_linfo, c->d_info + b.m0);
    return NEGF_OK;
}

// a step that a caller of a factor sweep does not need
const auto rgf_no_step = [](int, const cplx*) {};

// Level i of a factor sweep: D = A_ii - C_{i,i-1} g_{i-1} C_{i-1,i} - the layer's terminals (level 0: no Schur term),
// the caller's step before(i, D) on it, the inverse in place with B as its second area: *g = D or B, where g_i lies.
template <class Before>
int rgf_factor_level(const RgfBatch& b, const RgfView& v, int i, const cplx* gprev, cplx* D, cplx* B, Before& before, cplx** g)
{
    const RgfAreas& a = b.a;
    if (i > 0) {
        const int ni = v.n(i), np = v.n(i - 1);
        v.couplings(b, i - 1);
        rgf_mm(b, ni, np, np, a.CL, gprev, a.U);                       // C_{i,i-1} g_{i-1}
        rgf_mm(b, ni, ni, np, a.U, a.CU, a.V);                         // ... C_{i-1,i}
    }
    rgf_assemble_diag(b, v.layer(i), i > 0 ? a.V : nullptr, D);
    before(i, D);
    return rgf_inverse(b, v.layer(i), D, B, g);
}

// Factor sweep with every g_i kept in d_gstore, for the solve sweep that follows.  after(i, g_i) runs with CU, CL of the
// levels (i-1, i) still standing.
template <class Before, class After>
int rgf_factor_sweep(const RgfBatch& b, const RgfView& v, Before&& before, After&& after)
{
    const size_t layer_bytes = (size_t)b.nb * b.ls->stride * sizeof(cplx);
    for (int i = 0; i < b.ls->L; ++i) {
        cplx *D = b.g(i), *g = nullptr;
        int rc = rgf_factor_level(b, v, i, i > 0 ? b.g(i - 1) : nullptr, D, b.a.Glo, before, &g);
        if (rc) return rc;
        if (g != D) NEGF_HIP_CHECK(hipMemcpyAsync(D, g, layer_bytes, hipMemcpyDeviceToDevice, b.c->stream));
        after(i, D);
    }
    return NEGF_OK;
}

// Factor sweep that keeps only g_{i-1} alive and carries a corner block along: X_i = G_{i,0} (lower) or Y_i = G_{0,i}.
// Returns the block of the last level in *corner.  No solve sweep follows, so the solve sweep's areas are lent out
// here: W | Gup | Glo rotate as g_{i-1} | matrix to invert | second area, Gii[0] | Gii[1] alternate as the corner block.
int rgf_corner_sweep(const RgfBatch& b, bool lower, cplx** corner)
{
    const RgfAreas& a = b.a;
    const RgfView v{b.ls, false};
    const size_t layer_bytes = (size_t)b.nb * b.ls->stride * sizeof(cplx);
    cplx* const R[3] = {a.W, a.Gup, a.Glo};
    cplx *Xa = a.Gii[0], *Xb = a.Gii[1];
    cplx* gprev = nullptr;
    const int n0 = v.n(0);
    for (int i = 0; i < b.ls->L; ++i) {
        cplx* fr[3]; int k = 0;
        for (cplx* q : R) if (q != gprev) fr[k++] = q;                 // the areas g_{i-1} does not occupy
        cplx* g = nullptr;
        int rc = rgf_factor_level(b, v, i, gprev, fr[0], fr[1], rgf_no_step, &g);
        if (rc) return rc;
        const int ni = v.n(i);
        if (i == 0) { NEGF_HIP_CHECK(hipMemcpyAsync(Xa, g, layer_bytes, hipMemcpyDeviceToDevice, b.c->stream)); }
        else {
            if (lower) {
                rgf_mm(b, ni, n0, v.n(i - 1), a.CL, Xa, a.U);          // C_{i,i-1} X_{i-1}
                rgf_mm(b, ni, n0, ni, g, a.U, Xb);                     // X_i = g_i ...
            } else {
                rgf_mm(b, n0, ni, v.n(i - 1), Xa, a.CU, a.U);          // Y_{i-1} C_{i-1,i}
                rgf_mm(b, n0, ni, ni, a.U, g, Xb);                     // Y_i = ... g_i
            }
            std::swap(Xa, Xb);
        }
        gprev = g;
    }
    *corner = Xa;
    return NEGF_OK;
}

// What stands when a solve sweep calls its visitor at level i: G_ii, and below the last level U_i = g_i C_{i,i+1},
// G_{i,i+1} and -- for a visitor that wants_lower -- G_{i+1,i}.  The visitor may overwrite V, W and spare.
struct RgfLevel {
    int i;
    const cplx *Gii, *U, *Gup, *Glo;
};

// Solve sweep over the kept g_i, from the last level down; visitor.level(batch, RgfLevel) consumes each level as it stands
template <class Visitor>
int rgf_solve_sweep(const RgfBatch& b, const RgfView& v, Visitor&& visitor)
{
    constexpr bool lower = std::remove_reference<Visitor>::type::wants_lower;
    const RgfAreas& a = b.a;
    const int L = b.ls->L;
    const size_t s = b.ls->stride;
    const cplx* Gnext = b.g(L - 1);                                 // G of the last level is its g
    visitor.level(b, RgfLevel{L - 1, Gnext, nullptr, nullptr, nullptr});
    for (int i = L - 2; i >= 0; --i) {
        const int ni = v.n(i), nn = v.n(i + 1);
        const cplx* g = b.g(i);
        cplx* Gii = a.Gii[(L - i) & 1];
        v.couplings(b, i);
        rgf_mm(b, ni, nn, ni, g, a.CU, a.U);                           // U = g_i C_{i,i+1}
        rgf_mm(b, ni, nn, nn, a.U, Gnext, a.Gup);                      // G_{i,i+1}
        rgf_mm(b, nn, ni, ni, a.CL, g, a.V);                           // V = C_{i+1,i} g_i
        if (lower) rgf_mm(b, nn, ni, nn, Gnext, a.V, a.Glo);           // G_{i+1,i}
        rgf_mm(b, ni, ni, nn, a.Gup, a.V, a.W);                        // g_i C G_{i+1,i+1} C g_i
        { ProfScope ps(b.c, "rgf"); launch_rgf_add(b.c->stream, ni * ni, b.nb, g, s, a.W, s, Gii, s); }
        visitor.level(b, RgfLevel{i, Gii, a.U, a.Gup, lower ? a.Glo : nullptr});
        Gnext = Gii;
    }
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

// The two block visitors: level() takes G_ii, G_{i,i+1}, G_{i+1,i} of a Green's function sweep, less() a block A_ii or
// (up) A_{i,i+1} of G Gamma G^H from the column visitor.  This one sums them with the weights into the block lists on the
// pattern of S (gr_int, gless_int) ...
struct RgfSumBlocks {
    static constexpr bool wants_lower = true;
    const cplx* w;
    cplx* out;                                                          // diagonal | upper | lower blocks
    void level(const RgfBatch& b, const RgfLevel& lv) const
    {
        ProfScope ps(b.c, "accumulate");
        const LayeredSystem* ls = b.ls;
        const size_t s = ls->stride;
        const int i = lv.i;
        launch_rgf_accumulate(b.c->stream, ls->n[i] * ls->n[i], b.nb, w + b.m0, lv.Gii, s, out + ls->doff[i]);
        if (lv.Gup) {
            const int cnt = ls->n[i] * ls->n[i + 1];
            launch_rgf_accumulate(b.c->stream, cnt, b.nb, w + b.m0, lv.Gup, s, out + ls->dtot + ls->uoff[i]);
            launch_rgf_accumulate(b.c->stream, cnt, b.nb, w + b.m0, lv.Glo, s, out + ls->dtot + ls->utot + ls->uoff[i]);
        }
    }
    void less(const RgfBatch& b, int i, const cplx* A, bool up) const
    {
        ProfScope ps(b.c, "accumulate");
        const LayeredSystem* ls = b.ls;
        const size_t s = ls->stride;
        if (!up) { launch_rgf_accumulate(b.c->stream, ls->n[i] * ls->n[i], b.nb, w + b.m0, A, s, out + ls->doff[i]); return; }
        launch_rgf_accumulate(b.c->stream, ls->n[i] * ls->n[i + 1], b.nb, w + b.m0, A, s, out + ls->dtot + ls->uoff[i]);
        // the lower block (i+1, i): sum_k w_k conj(A_{i,i+1}(E_k))^T
        launch_rgf_accumulate_ct(b.c->stream, ls->n[i], ls->n[i + 1], b.nb, w + b.m0, A, s, out + ls->dtot + ls->utot + ls->uoff[i]);
    }
};

// ... this one reduces them to the per-site densities [m][N] on the device (dos, contact_dos)
struct RgfDosBlocks {
    static constexpr bool wants_lower = true;
    int form;                                                           // of level(): 0 diag G, 1 diag(G S)
    double* site;
    void level(const RgfBatch& b, const RgfLevel& lv) const
    {
        ProfScope ps(b.c, "rgf");
        const LayeredSystem* ls = b.ls;
        const size_t s = ls->stride, N = (size_t)ls->N;
        const int i = lv.i;
        double* row = site + (size_t)b.m0 * N;
        if (form == 0) { launch_rgf_dos_diag(b.c->stream, ls->n[i], b.nb, lv.Gii, s, row + ls->off[i], N); return; }
        // -Im (G S)_rr / pi, S_kr read as conj(S_rk): the diagonal block, then the two neighbours
        launch_rgf_dos_rows(b.c->stream, ls->n[i], ls->n[i], b.nb, lv.Gii, s, ls->dSd + ls->doff[i], row + ls->off[i], N, false);
        if (lv.Gup) {
            launch_rgf_dos_rows(b.c->stream, ls->n[i], ls->n[i + 1], b.nb, lv.Gup, s, ls->dSu + ls->uoff[i], row + ls->off[i], N, true);
            launch_rgf_dos_rows(b.c->stream, ls->n[i + 1], ls->n[i], b.nb, lv.Glo, s, ls->dSl + ls->uoff[i], row + ls->off[i + 1], N, true);
        }
    }
    void less(const RgfBatch& b, int i, const cplx* A, bool up) const
    {
        ProfScope ps(b.c, "rgf");
        const LayeredSystem* ls = b.ls;
        const size_t s = ls->stride, N = (size_t)ls->N;
        double* row = site + (size_t)b.m0 * N;
        if (!up) launch_rgf_pop_block(b.c->stream, ls->n[i], ls->n[i], b.nb, A, s, ls->dSd + ls->doff[i], row + ls->off[i], false, nullptr, N);
        // the rows of layer i, and through A_{i+1,i} = A_{i,i+1}^H the rows of layer i + 1 as the block's column sums
        else launch_rgf_pop_block(b.c->stream, ls->n[i], ls->n[i + 1], b.nb, A, s, ls->dSu + ls->uoff[i], row + ls->off[i], true,
                                  row + ls->off[i + 1], N);
    }
};

// The groups of a bond-table call: g[i] groups on layer i, the tables' block offsets in negf_layered_gr_int's order with g
// in place of n, and on the device per layer the orbitals sorted by group (perm, at off[i]) and the groups' offsets in
// that list (goff, at gat[i]).  Without a map (orbital level) g = n and nothing is uploaded.
struct RgfBondGroups {
    bool mapped = false;
    std::vector<int> g, gat;
    std::vector<size_t> doff, uoff;
    size_t dtot = 0, utot = 0;
    std::vector<int> map;                                               // host: perm [N] | goff [sum (g_i + 1)]
    const int* d_map = nullptr;
    size_t table() const { return dtot + 2 * utot; }                    // doubles per energy
};

// validation and the host tables of the groups; NEGF_EINVAL before anything is launched
int rgf_bond_groups(const LayeredSystem* ls, const int* groups_per_layer, const int* group_of, RgfBondGroups* bg)
{
    if ((groups_per_layer == nullptr) != (group_of == nullptr)) return NEGF_EINVAL;
    const int L = ls->L;
    bg->mapped = group_of != nullptr;
    bg->g.assign(ls->n.begin(), ls->n.end());
    if (bg->mapped)
        for (int i = 0; i < L; ++i) {
            if (groups_per_layer[i] < 1) return NEGF_EINVAL;
            bg->g[i] = groups_per_layer[i];
            for (int o = ls->off[i]; o < ls->off[i] + ls->n[i]; ++o)
                if (group_of[o] < 0 || group_of[o] >= bg->g[i]) return NEGF_EINVAL;
        }
    bg->doff.resize(L); bg->uoff.resize(L - 1);
    for (int i = 0; i < L; ++i) {
        bg->doff[i] = bg->dtot; bg->dtot += (size_t)bg->g[i] * bg->g[i];
        if (i + 1 < L) { bg->uoff[i] = bg->utot; bg->utot += (size_t)bg->g[i] * bg->g[i + 1]; }
    }
    if (!bg->mapped) return NEGF_OK;
    bg->gat.resize(L);
    size_t at = (size_t)ls->N;
    for (int i = 0; i < L; ++i) { bg->gat[i] = (int)at; at += (size_t)bg->g[i] + 1; }
    bg->map.assign(at, 0);
    for (int i = 0; i < L; ++i) {                                       // a counting sort per layer: ascending inside a group
        int* perm = bg->map.data() + ls->off[i];
        int* goff = bg->map.data() + bg->gat[i];
        const int* go = group_of + ls->off[i];
        for (int o = 0; o < ls->n[i]; ++o) ++goff[go[o] + 1];
        for (int k = 0; k < bg->g[i]; ++k) goff[k + 1] += goff[k];
        std::vector<int> next(goff, goff + bg->g[i]);
        for (int o = 0; o < ls->n[i]; ++o) perm[next[go[o]]++] = o;
    }
    return NEGF_OK;
}

// ... and this one, which stands behind the column visitor only (less(); no Green's function sweep feeds it), turns the
// blocks of A = G Gamma G^H into the flow 2 Im[K conj(A)], K = E S - F, where RgfSumBlocks::less would sum them: per energy
// at orbital level or as group tables (negf_layered_local_transmission; w null), or summed with real weights
// (negf_layered_bond_int).  The lower block (i+1, i) comes from the upper A read transposed: A_{i+1,i} is never formed.
struct RgfBondBlocks {
    const double* w;                                                    // null: per-energy tables
    double* out;                                                        // diagonal | upper | lower, [m] of those without w
    const RgfBondGroups* bg;
    void less(const RgfBatch& b, int i, const cplx* A, bool up) const
    {
        ProfScope ps(b.c, "bond");
        const LayeredSystem* ls = b.ls;
        hipStream_t st = b.c->stream;
        const size_t s = ls->stride;
        const cplx* E = b.E + b.m0;
        const int ni = ls->n[i], nb = b.nb;
        const cplx *S = up ? ls->dSu + ls->uoff[i] : ls->dSd + ls->doff[i], *F = up ? ls->dFu + ls->uoff[i] : ls->dFd + ls->doff[i];
        const int nc = up ? ls->n[i + 1] : ni;
        const size_t at = up ? bg->dtot + bg->uoff[i] : bg->doff[i];   // the block's place in a table; the lower one's: + utot
        // A_ii = (W Gamma) W^H is Hermitian to the rounding of its products only; the flow of a diagonal block reads its
        // Hermitian part, formed in place (the block lies in one of the column visitor's own areas, which nobody reads
        // again), so that at real E flow_ii is antisymmetric bit for bit as the coupling blocks' flows are
        if (!up) launch_rgf_bond_hermitize(st, ni, nb, const_cast<cplx*>(A), s);
        if (w) {
            launch_rgf_bond_accumulate(st, ni * nc, nb, E, w + b.m0, S, F, A, s, out + at);
            if (up) launch_rgf_bond_accumulate_t(st, ni, nc, nb, E, w + b.m0, ls->dSl + ls->uoff[i], ls->dFl + ls->uoff[i], A, s,
                                                 out + at + bg->utot);
            return;
        }
        const size_t tab = bg->table();
        double* o = out + tab * b.m0 + at;
        const int* info = b.c->d_info + b.m0;
        if (!bg->mapped) {
            launch_rgf_bond_flow(st, ni * nc, nb, E, S, F, A, s, info, o, tab);
            if (up) launch_rgf_bond_flow_t(st, ni, nc, nb, E, ls->dSl + ls->uoff[i], ls->dFl + ls->uoff[i], A, s, info, o + bg->utot, tab);
            return;
        }
        const int j = up ? i + 1 : i;
        const int *rperm = bg->d_map + ls->off[i], *rgoff = bg->d_map + bg->gat[i];
        const int *cperm = bg->d_map + ls->off[j], *cgoff = bg->d_map + bg->gat[j];
        launch_rgf_bond_group(st, nc, bg->g[i], bg->g[j], nb, false, E, S, F, A, s, info, rperm, rgoff, cperm, cgoff, o, tab);
        if (up) launch_rgf_bond_group(st, nc, bg->g[i], bg->g[j], nb, true, E, S, F, A, s, info, rperm, rgoff, cperm, cgoff, o + bg->utot, tab);
    }
};

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
    RgfCarve cols{r.ls->d_cols.p};
    if (less->K[0] > 0) {
        less->z = cols.take((size_t)(r.ls->L - 1) * cb);
        less->x[0] = cols.take(cb); less->x[1] = cols.take(cb);
    }
    for (int e = 0; e < 2; ++e) {
        if (less->K[e] == 0) continue;
        less->W[e][0] = cols.take(cb); less->W[e][1] = cols.take(cb); less->Y[e] = cols.take(cb);
        less->gam[e] = cols.take((size_t)less->K[e] * less->K[e] * r.nb_max);
    }
}

// The factor sweep's part in G Gamma G^H, after the inverse of level i: the x / z chain of the column set on layer 0
void rgf_less_chain(const RgfBatch& b, RgfLess* less, int i, const cplx* g)
{
    const int K = less->K[0];
    if (K == 0) return;
    const LayeredSystem* ls = b.ls;
    const size_t s = ls->stride, cs = less->cs;
    const int ni = ls->n[i];
    if (i == 0) { ProfScope ps(b.c, "rgf"); launch_rgf_gather_cols(b.c->stream, ni, K, b.nb, g, s, less->J[0], less->x[0], cs); return; }
    cplx* z = less->z + (size_t)(i - 1) * b.nb_max * cs;
    ProfScope ps(b.c, "zgemm");
    launch_zgemm(b.c->stream, ni, K, ls->n[i - 1], b.nb, b.a.CL, ls->n[i - 1], s, less->x[0], K, cs, 0, z, K, cs);   // z_i = C_{i,i-1} x_{i-1}
    if (i + 1 < ls->L) {
        launch_zgemm(b.c->stream, ni, K, ni, b.nb, g, ni, s, z, K, cs, 0, less->x[1], K, cs);                         // x_i = g_i z_i
        std::swap(less->x[0], less->x[1]);
    }
}

// The column visitor: the columns W_i of each selected end from G_ii, U_i and W_{i+1}, then the blocks A_ii and A_{i,i+1}
// (the layer-0 set's contribution first, the last layer's added to it) handed to a block visitor's less() one after the other.
template <class Blocks>
struct RgfColumns {
    static constexpr bool wants_lower = false;
    RgfLess* less;
    const Blocks& sink;
    void level(const RgfBatch& b, const RgfLevel& lv)
    {
        const LayeredSystem* ls = b.ls;
        hipStream_t st = b.c->stream;
        const size_t s = ls->stride, cs = less->cs;
        const int i = lv.i, nb = b.nb, ni = ls->n[i], L = ls->L;
        for (int e = 0; e < 2; ++e) {
            const int K = less->K[e];
            if (K == 0) continue;
            cplx* W = less->W[e][1];
            if ((e == 0 && i == 0) || (e == 1 && i == L - 1)) {
                ProfScope ps(b.c, "rgf");
                launch_rgf_gather_cols(st, ni, K, nb, lv.Gii, s, less->J[e], W, cs);
            } else if (e == 0) {
                ProfScope ps(b.c, "zgemm");
                launch_zgemm(st, ni, K, ni, nb, lv.Gii, ni, s, less->z + (size_t)(i - 1) * b.nb_max * cs, K, cs, 0, W, K, cs);   // G_ii z_i
            } else {
                const int nn = ls->n[i + 1];
                ProfScope ps(b.c, "zgemm");
                launch_zgemm(st, ni, K, nn, nb, lv.U, nn, s, less->W[e][0], K, cs, 0, W, K, cs);                                  // U_i W_{i+1}
            }
            ProfScope ps(b.c, "zgemm");
            launch_zgemm(st, ni, K, K, nb, W, K, cs, less->gam[e], K, (size_t)K * K, 0, less->Y[e], K, cs);                       // Y_i = W_i Gamma
        }
        // G_ii stands and U has been read: the two ends' block products go to spare and W, their sum to V
        const RgfAreas& a = b.a;
        cplx* const Ab[2] = {a.spare, a.W};
        cplx* const Asum = a.V;
        const bool both = less->K[0] > 0 && less->K[1] > 0;
        for (int up = 0; up < 2; ++up) {
            if (up && i == L - 1) break;
            const int nc = up ? ls->n[i + 1] : ni;
            for (int e = 0; e < 2; ++e) {
                const int K = less->K[e];
                if (K == 0) continue;
                ProfScope ps(b.c, "zgemm");
                // op(B) = W^H; the diagonal block is a Hermitian product
                launch_zgemm(st, ni, nc, K, nb, less->Y[e], K, cs, less->W[e][up ? 0 : 1], K, cs, up ? 1 : 3, Ab[e], nc, s);
            }
            const cplx* A = less->K[0] > 0 ? Ab[0] : Ab[1];
            if (both) { ProfScope ps(b.c, "rgf"); launch_rgf_add(st, ni * nc, nb, Ab[0], s, Ab[1], s, Asum, s); A = Asum; }
            sink.less(b, i, A, up != 0);
        }
        for (int e = 0; e < 2; ++e) std::swap(less->W[e][0], less->W[e][1]);       // W_i is the next level's W_{i+1}
    }
};

// One batch of a call on the pattern of S.  Without `less` the two sweeps of the Green's function, its blocks to the block
// visitor; with it G Gamma G^H (rgf_less_batch, which asks of the block visitor its less() only): factor sweep with the
// layer-0 chain, the Gamma of the selected terminals on their union lists, solve sweep with the column visitor in front of
// the block visitor
template <class Blocks>
int rgf_less_batch(const RgfBatch& b, RgfLess* less, const Blocks& sink)
{
    const RgfView v{b.ls, false};
    int rc;
    if ((rc = rgf_factor_sweep(b, v, rgf_no_step, [&](int i, const cplx* g) { rgf_less_chain(b, less, i, g); }))) return rc;
    {
        ProfScope ps(b.c, "gamma");
        for (int e = 0; e < 2; ++e)
            if (less->K[e] > 0)
                launch_rgf_gamma_union(b.c->stream, less->K[e], b.nb, less->J[e], rgf_term_args(b.ls, e, b.m0, less->only), less->gam[e],
                                       (size_t)less->K[e] * less->K[e]);
    }
    return rgf_solve_sweep(b, v, RgfColumns<Blocks>{less, sink});
}

template <class Blocks>
int rgf_pattern_batch(const RgfBatch& b, RgfLess* less, const Blocks& sink)
{
    if (less) return rgf_less_batch(b, less, sink);
    const RgfView v{b.ls, false};
    const int rc = rgf_factor_sweep(b, v, rgf_no_step, rgf_no_step);
    return rc ? rc : rgf_solve_sweep(b, v, sink);
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
    // where a visitor finds the columns of terminal b in the strip of a pass, and the strip's first column
    struct Cols { const int* d_tcol; const std::vector<int>* tcol; int col0; };
    Cols alternating(int pass, int layer) const { return Cols{d_tcol[pass], &tcol[pass], colbase[pass][layer]}; }
    Cols kept() const { return Cols{d_tcol[0], &tcol[0], 0}; }           // a kept strip has all K_tot columns, ascending in q
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
    // the probes of each layer in the dense path's content order (inside a layer, local and global orbital numbers order alike)
    pl->poff.assign(L + 1, 0);
    for (int q = 0; q < L; ++q) {
        pl->poff[q] = (int)pl->porder.size();
        const size_t at = pl->porder.size();
        for (int t : on[q]) if (t >= nt) pl->porder.push_back(t);
        std::stable_sort(pl->porder.begin() + at, pl->porder.end(),
                         [&](int a, int b) { return tmat_probe_before(pl->K, pl->rows, pl->ioff, psig, pl->soff, a, b); });
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

// the pairs of view level i of a pass, read from the level's strip (n x ld) whose columns `at` describes
void rgf_tmat_pairs(negf_ctx* c, LayeredSystem* ls, const RgfTmatPlan& pl, int pass, int i, int nb, const cplx* strip, int ld,
                    const RgfTmatPlan::Cols& at, double* T)
{
    const int L = ls->L, C = pl.C;
    const int col0 = at.col0;
    const size_t k0 = ((size_t)pass * L + i) * 3;
    if (pl.pair_n[k0] + pl.pair_n[k0 + 1] + pl.pair_n[k0 + 2] == 0) return;
    ProfScope ps(c, "tmat");
    double cmadds = 0;
    for (int cls = 1; cls <= 2; ++cls) {
        launch_rgf_strip_pairs(c->stream, cls, C, pl.pair_n[k0 + cls], pl.max_elems[cls], nb, pl.d_pairs + pl.pair_at[k0 + cls],
                               pl.dK, pl.d_ioff, pl.d_goff, pl.d_gstride, at.d_tcol, col0, pl.d_rows, pl.d_cpos, strip, ld,
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
        launch_gather_block(c->stream, ld, Ka, Kb, nb, strip + ((*at.tcol)[b] - col0), pl.cs, pl.d_rows + pl.ioff[a],
                            pl.d_cpos + pl.ioff[b], pl.Gab, kk);
        launch_zgemm(c->stream, Ka, Kb, Ka, nb, ga, Ka, (size_t)pl.gstride[a], pl.Gab, Kb, kk, 0, pl.Xs, Kb, kk);
        launch_zgemm(c->stream, Ka, Kb, Kb, nb, pl.Xs, Kb, kk, gb, Kb, (size_t)pl.gstride[b], 0, pl.Ys, Kb, kk);
        launch_trace_dot(c->stream, Ka, Kb, nb, pl.Ys, Kb, kk, pl.Gab, Kb, kk, T + (size_t)a * C + b, C * C);
    }
}

// The level code of the strip visitors.  The strip of view level i (n_i rows at the leading dimension ld, batch stride
// pl.cs) is the columns J of its own layer cut from G_ii -- the head, nhead columns from column `head` on -- and
// U_i times wtail columns of the strip of level i + 1 (src, leading dimension src_ld) from column `tail` on.
void rgf_strip_level(const RgfBatch& b, const RgfView& v, const RgfTmatPlan& pl, const RgfLevel& lv, cplx* dst, int ld, int head,
                     int nhead, int tail, const cplx* src, int src_ld, int wtail)
{
    const int i = lv.i, ni = v.n(i);
    if (wtail > 0) {
        const int nn = v.n(i + 1);
        ProfScope ps(b.c, "zgemm");
        launch_zgemm(b.c->stream, ni, wtail, nn, b.nb, lv.U, nn, b.ls->stride, src, src_ld, pl.cs, 0, dst + tail, ld, pl.cs);
    }
    if (nhead > 0) {
        ProfScope ps(b.c, "rgf");
        launch_rgf_strip_head(b.c->stream, ni, nhead, ld, b.nb, lv.Gii, b.ls->stride, pl.d_J + pl.Joff[v.layer(i)], dst + head, pl.cs);
    }
}

// The strip visitor of the transmission matrix: strip_i = [G_ii[:, J_i] | U_i strip_{i+1}] in one of the two alternating
// strip areas, then the pairs of the level read from it; the strip of level i + 1 is dropped
struct RgfStrips {
    static constexpr bool wants_lower = false;
    const RgfView& v;
    const RgfTmatPlan& pl;
    double* T;
    cplx *Scur, *Snext;
    int wnext = 0;                                                     // width of the strip of level i + 1
    void level(const RgfBatch& b, const RgfLevel& lv)
    {
        const int i = lv.i, p = v.layer(i), nj = pl.nJ[p], w = nj + wnext;
        rgf_strip_level(b, v, pl, lv, Scur, w, 0, nj, nj, Snext, wnext, wnext);
        rgf_tmat_pairs(b.c, b.ls, pl, v.reversed, i, b.nb, Scur, w, pl.alternating(v.reversed, p), T);
        std::swap(Scur, Snext);
        wnext = w;
    }
};

// The strip visitor of the floating-probe calls, which need the strips of ALL layers once D is known: layer p's strip lives
// in keep [L][nb_max][cs] as the n_p x K_tot matrix Cfull_p = [G_{p,q}[:, J_q]]_q with the column blocks in ascending q (J_q
// at column Joff[q]).  The pass over the layers as they are writes the blocks q >= p -- the head and U_p times the same
// columns of Cfull_{p+1} --, the reversed pass, which runs second, the blocks q < p as U_p times those columns of
// Cfull_{p-1}: the same-layer block stays the first pass's, as the pairs of one layer are.  T null: no pairs (the total).
struct RgfKeptStrips {
    static constexpr bool wants_lower = false;
    const RgfView& v;
    const RgfTmatPlan& pl;
    double* T;
    cplx* keep;
    cplx* at(const RgfBatch& b, int layer) const { return keep + (size_t)layer * b.nb_max * pl.cs; }
    void level(const RgfBatch& b, const RgfLevel& lv)
    {
        const int i = lv.i, p = v.layer(i), L = b.ls->L, Kt = pl.Ktot;
        cplx* dst = at(b, p);
        if (!v.reversed) {
            const int tail = pl.Joff[p] + pl.nJ[p];
            rgf_strip_level(b, v, pl, lv, dst, Kt, pl.Joff[p], pl.nJ[p], tail, p + 1 < L ? at(b, p + 1) + tail : nullptr, Kt,
                            p + 1 < L ? Kt - tail : 0);
        } else {
            rgf_strip_level(b, v, pl, lv, dst, Kt, 0, 0, 0, p > 0 ? at(b, p - 1) : nullptr, Kt, p > 0 ? pl.Joff[p] : 0);
        }
        if (T) rgf_tmat_pairs(b.c, b.ls, pl, v.reversed, i, b.nb, dst, Kt, pl.kept(), T);
    }
};

// the probes of a level's layer taken out of its diagonal before the inverse: the `before` step of a factor sweep
auto rgf_sub_probes_step(const RgfBatch& b, const RgfView& v, const RgfTmatPlan& pl)
{
    return [&b, v, &pl](int i, cplx* D) {
        const int p = v.layer(i), np = pl.poff[p + 1] - pl.poff[p];
        if (np == 0) return;
        ProfScope ps(b.c, "rgf");
        launch_rgf_sub_probes(b.c->stream, v.n(i), np, b.nb, pl.d_porder + pl.poff[p], pl.dK, pl.d_ioff, pl.d_soff, pl.d_rows,
                              b.ls->d_tm_sig, D, b.ls->stride);
    };
}

// One pass of a batch: factor sweep with the probes in the diagonal, solve sweep with a strip visitor -- the pairs (a, b)
// with b on a's level or a later one of the view
template <class Strips>
int rgf_tmat_pass(const RgfBatch& b, const RgfTmatPlan& pl, const RgfView& v, Strips&& strips)
{
    int rc = rgf_factor_sweep(b, v, rgf_sub_probes_step(b, v, pl), rgf_no_step);
    return rc ? rc : rgf_solve_sweep(b, v, strips);
}

// The Gamma blocks that depend on E, of the batch
void rgf_tmat_gamma_dyn(const RgfBatch& b, const RgfTmatPlan& pl)
{
    ProfScope ps(b.c, "tmat");
    for (int t = 0; t < pl.nt; ++t) {
        if (b.ls->terms[t]->kind == 0) continue;
        const cplx* sig; size_t st;
        rgf_sigma_of(b.ls->terms[t], b.m0, &sig, &st);
        launch_rgf_gamma(b.c->stream, pl.K[t], b.nb, sig, st, pl.gdyn + pl.goff[t], pl.dyn);
    }
}

// T [nb][C][C] of one batch of a transmission-matrix call: the two passes with alternating strips, NaN for singular energies
int rgf_tmat_batch(const RgfBatch& b, const RgfTmatPlan& pl, double* T)
{
    rgf_tmat_gamma_dyn(b, pl);
    for (int pass = 0; pass < (pl.two_pass ? 2 : 1); ++pass) {
        const RgfView v{b.ls, pass == 1};
        if (int e = rgf_tmat_pass(b, pl, v, RgfStrips{v, pl, T, pl.strip[0], pl.strip[1]})) return e;
    }
    ProfScope ps(b.c, "tmat");
    launch_tmat_nan(b.c->stream, pl.C, b.nb, b.c->d_info + b.m0, T);
    return NEGF_OK;
}

// work areas of a transmission-matrix batch, out of d_cols
void rgf_tmat_layout(const RgfRun& r, RgfTmatPlan* pl, RgfCarve* cols)
{
    const size_t nbm = (size_t)r.nb_max;
    pl->strip[0] = cols->take(pl->cs * nbm); pl->strip[1] = cols->take(pl->cs * nbm);
    pl->gdyn = cols->take(pl->dyn * nbm);
    pl->Gab = cols->take(pl->big_kk * nbm); pl->Xs = cols->take(pl->big_kk * nbm); pl->Ys = cols->take(pl->big_kk * nbm);
}

// The batches of a device-resident call, once its work areas stand: per batch its info cleared and the Sigma blocks of
// the chain terminals evaluated into their d_blk, then body(batch)
template <class Body>
int rgf_batches(const RgfRun& r, int m, const double* E_dev, Body&& body)
{
    negf_ctx* c = r.c;
    int rc;
    for (int m0 = 0; m0 < m; m0 += r.nb_max) {
        const RgfBatch b{r, m0, std::min(r.nb_max, m - m0), reinterpret_cast<const cplx*>(E_dev)};
        NEGF_HIP_CHECK(hipMemsetAsync(c->d_info + m0, 0, (size_t)b.nb * sizeof(int), c->stream));
        for (auto* t : r.ls->terms)
            if (t->kind == 1 && (rc = run_sigma_blocks(c, t->chain, b.nb, b.E + m0, r.ls->d_iters, r.ls->d_conv, m0, t->d_blk.p))) return rc;
        if ((rc = body(b))) return rc;
    }
    return close_call(c, m);
}

// ------------------------------------------------- floating probes on layers: G D G^H on the pattern of S
// What negf_layered_gless_int_probes adds to the plan of a transmission-matrix call.  D_s = scatter(Gamma_s) + sum_p R_ps
// scatter(Gamma_p) is block diagonal over the layers (every terminal lives in one): D_q on J_q, the blocks one after the
// other per energy.  R needs the whole T, hence both passes, before D exists: the strips of ALL layers are kept
// (RgfKeptStrips), then Y_i = Cfull_i blockdiag(D_q) in one launch, A_ii = Y_i Cfull_i^H, A_{i,i+1} = Y_i Cfull_{i+1}^H.
struct RgfDephPlan {
    int contact = -1;                                                   // the column of R; -1: the total, every weight 1
    bool floating = false;                                              // a contact and probes: T and R are needed
    std::vector<int> sel;                                               // the end terminals that enter D, in the order they were made
    size_t Dtot = 0, per_energy = 0;
    int nct = 0;                                                        // column tiles of the block-diagonal product
    const int *d_sel = nullptr, *d_tlayer = nullptr, *d_poff = nullptr, *d_nl = nullptr, *d_nJ = nullptr, *d_Joff = nullptr,
              *d_Doff = nullptr, *d_ctile = nullptr;
    std::vector<int> tab;
    size_t at[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    cplx *keep = nullptr, *Y = nullptr, *D = nullptr;                   // [L][batch][cs] twice, [batch][Dtot]
    double *T = nullptr, *R = nullptr;
};

// the host tables; NEGF_EINVAL (sizes beyond what one launch of the block-diagonal product indexes) before anything is launched
int rgf_deph_plan(const LayeredSystem* ls, const RgfTmatPlan& pl, int ind, RgfDephPlan* dp)
{
    const int L = ls->L, nt = pl.nt;
    dp->contact = ind == NEGF_IND_TOTAL ? -1 : (ind < 0 ? ind + nt : ind);
    dp->floating = dp->contact >= 0 && pl.n_probes > 0;
    for (int t = 0; t < nt; ++t) if (dp->contact < 0 || t == dp->contact) dp->sel.push_back(t);
    std::vector<int> Doff(L, 0), ctile;
    const int tj = rgf_blockdiag_tile_cols();
    size_t dtot = 0;
    for (int q = 0; q < L; ++q) {
        Doff[q] = (int)dtot;
        dtot += (size_t)pl.nJ[q] * pl.nJ[q];
        if (dtot > ((size_t)1 << 30)) return NEGF_EINVAL;
        for (int t = 0; t < rgf_blockdiag_col_tiles(pl.nJ[q]); ++t) { ctile.push_back(q); ctile.push_back(t * tj); }
    }
    dp->Dtot = dtot;
    dp->nct = (int)(ctile.size() / 2);
    if ((double)L * rgf_blockdiag_row_tiles(ls->nmax) * dp->nct > 2.0e9) return NEGF_EINVAL;
    int k = 0;
    const std::vector<int>* const parts[8] = {&dp->sel, &pl.layer, &pl.poff, &ls->n, &pl.nJ, &pl.Joff, &Doff, &ctile};
    for (const std::vector<int>* v : parts) {
        dp->at[k++] = dp->tab.size();
        dp->tab.insert(dp->tab.end(), v->begin(), v->end());
    }
    // per energy in flight: the kept strips and Y of all layers, the Gamma blocks that depend on E, G_ab | X | Y of the
    // class-0 pairs, D
    dp->per_energy = 2 * (size_t)L * pl.cs + pl.dyn + 3 * pl.big_kk + dtot;
    return NEGF_OK;
}

int rgf_deph_setup(negf_ctx* c, LayeredSystem* ls, const RgfTmatPlan& pl, const RgfRun& r, RgfDephPlan* dp)
{
    int rc;
    if ((rc = ensure_cap(c, ls->d_deph_tab, dp->tab.size() + 1)) || (rc = upload(c, ls->d_deph_tab.p, dp->tab.data(), dp->tab.size()))) return rc;
    const int* d = ls->d_deph_tab;
    dp->d_sel = d + dp->at[0]; dp->d_tlayer = d + dp->at[1]; dp->d_poff = d + dp->at[2]; dp->d_nl = d + dp->at[3];
    dp->d_nJ = d + dp->at[4]; dp->d_Joff = d + dp->at[5]; dp->d_Doff = d + dp->at[6]; dp->d_ctile = d + dp->at[7];
    const size_t nbm = (size_t)r.nb_max;
    if (dp->floating) {
        if ((rc = ensure_cap(c, ls->d_deph_T, (size_t)pl.C * pl.C * nbm)) ||
            (rc = ensure_cap(c, ls->d_deph_R, (size_t)pl.n_probes * pl.nt * nbm))) return rc;
        dp->T = ls->d_deph_T; dp->R = ls->d_deph_R;
    }
    return NEGF_OK;
}

// One batch: both passes with the strips kept (the pairs into T only when R is needed), R, D, Y, then layer by layer the
// blocks A_ii (a Hermitian product: D is exactly Hermitian) and A_{i,i+1} to the block visitor's less(), as RgfColumns hands them on
template <class Blocks>
int rgf_deph_batch(const RgfBatch& b, const RgfTmatPlan& pl, const RgfDephPlan& dp, const Blocks& sink)
{
    negf_ctx* c = b.c;
    const LayeredSystem* ls = b.ls;
    const int L = ls->L, Kt = pl.Ktot, nb = b.nb;
    rgf_tmat_gamma_dyn(b, pl);
    double* T = dp.floating ? dp.T : nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        const RgfView v{ls, pass == 1};
        if (int e = rgf_tmat_pass(b, pl, v, RgfKeptStrips{v, pl, T, dp.keep})) return e;
    }
    if (dp.floating) {
        { ProfScope ps(c, "tmat"); launch_tmat_nan(c->stream, pl.C, nb, c->d_info + b.m0, T); }
        if (int e = deph_run_response(c, pl.C, pl.nt, pl.d_porder, nb, T, dp.R)) return e;
    }
    {
        ProfScope ps(c, "deph");
        launch_rgf_deph_coupling(c->stream, L, nb, pl.nt, pl.n_probes, dp.floating ? dp.contact : -1, (int)dp.sel.size(), dp.d_sel,
                                 dp.d_tlayer, pl.d_porder, dp.d_poff, dp.d_nJ, dp.d_Doff, pl.dK, pl.d_ioff, pl.d_goff,
                                 pl.d_gstride, pl.d_cpos, ls->d_tm_gam, pl.gdyn, dp.R, dp.D, dp.Dtot);
        launch_rgf_blockdiag_mm(c->stream, L, ls->nmax, dp.nct, Kt, nb, b.nb_max, pl.cs, dp.d_nl, dp.d_nJ, dp.d_Joff, dp.d_Doff,
                                dp.d_ctile, dp.keep, dp.D, dp.Dtot, dp.Y);
        double kk = 0;
        for (int q = 0; q < L; ++q) kk += (double)pl.nJ[q] * pl.nJ[q];
        negf_count_flops(8.0 * (double)ls->N * kk * nb, 0.0);
    }
    const size_t s = ls->stride, lay = (size_t)b.nb_max * pl.cs;
    for (int i = L - 1; i >= 0; --i) {
        const int ni = ls->n[i];
        const cplx *Yi = dp.Y + lay * i, *Ci = dp.keep + lay * i;
        { ProfScope ps(c, "zgemm"); launch_zgemm(c->stream, ni, ni, Kt, nb, Yi, Kt, pl.cs, Ci, Kt, pl.cs, 3, b.a.Gup, ni, s); }
        sink.less(b, i, b.a.Gup, false);
        if (i + 1 == L) continue;
        const int nn = ls->n[i + 1];
        { ProfScope ps(c, "zgemm"); launch_zgemm(c->stream, ni, nn, Kt, nb, Yi, Kt, pl.cs, Ci + lay, Kt, pl.cs, 1, b.a.Glo, nn, s); }
        sink.less(b, i, b.a.Glo, true);
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
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, false, &r))) return rc;
    const int Ka = ta->K, Kb = tb->K;
    const size_t kab = (size_t)Ka * Kb, sa = (size_t)Ka * Ka, sb = (size_t)Kb * Kb, nbm = (size_t)r.nb_max;
    if ((rc = ensure_cap(c, ls->d_small, (sa + sb + 3 * kab) * nbm))) return rc;
    RgfCarve small{ls->d_small.p};
    cplx *gamA = small.take(sa * nbm), *gamB = small.take(sb * nbm);
    cplx *Gab = small.take(kab * nbm), *Xs = small.take(kab * nbm), *Ys = small.take(kab * nbm);
    // a on the last layer: G_ab is cut from G_{L-1,0} (X); a on layer 0: from G_{0,L-1} (Y)
    const bool lower = ta->end == 1;
    const int ld = lower ? ls->n[0] : ls->n[ls->L - 1];
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) {
        cplx* Gc = nullptr;
        if (int e = rgf_corner_sweep(b, lower, &Gc)) return e;
        const cplx *sA, *sB; size_t stA, stB;
        rgf_sigma_of(ta, b.m0, &sA, &stA); rgf_sigma_of(tb, b.m0, &sB, &stB);
        {
            ProfScope ps(c, "gamma");
            launch_rgf_gamma(c->stream, Ka, b.nb, sA, stA, gamA, sa);
            launch_rgf_gamma(c->stream, Kb, b.nb, sB, stB, gamB, sb);
        }
        {
            ProfScope ps(c, "zgemm");
            launch_gather_block(c->stream, ld, Ka, Kb, b.nb, Gc, ls->stride, ta->d_idx, tb->d_idx, Gab, kab);
            launch_zgemm(c->stream, Ka, Kb, Ka, b.nb, gamA, Ka, sa, Gab, Kb, kab, 0, Xs, Kb, kab);
            launch_zgemm(c->stream, Ka, Kb, Kb, b.nb, Xs, Kb, kab, gamB, Kb, sb, 0, Ys, Kb, kab);
        }
        ProfScope ps(c, "trace");
        launch_trace_dot(c->stream, Ka, Kb, b.nb, Ys, Kb, kab, Gab, Kb, kab, T_dev + b.m0, 1);
        return NEGF_OK;
    });
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
    if ((rc = negf_layered_transmission_dev(c, h, term_a, term_b, m, dev_E(c), c->d_scal))) return rc;
    return fetch_result_and_info(c, m, c->d_scal, (size_t)m * sizeof(double), T, info);
}

// ------------------------------------------------- transmission eigenchannels (include/negf_layered_channels.h)
// The dense channel call (negf_api.hip, ChanWork) on the corner block: s = the terminal with the shorter list (a unless
// K_b < K_a), Gamma_s = L L^H, Z = L^H G_so (the block is gathered as G[I_a, I_b] either way: with s = b it enters Z
// conjugate-transposed), W = Z Gamma_o, H = W Z^H, then the eigenvalues of H's leading rank x rank block.  Which kernels
// factor and diagonalise: those of k_channels.hip up to their K = 96, the wide ones (k_eig_wide.hip) above it or where
// negf_set_channel_algo(1) asks for them.
struct RgfChanPlan {
    RgfTerminal *ta, *tb;
    int Ks, Ko;
    bool mirror, wide, constant;                // constant: Gamma_s does not depend on E -- factored once per call
};

static int rgf_chan_plan(negf_ctx* c, int h, int term_a, int term_b, LayeredSystem** lsp, RgfChanPlan* pl)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls) return NEGF_EINVAL;
    const int nt = (int)ls->terms.size();
    if (term_a < 0 || term_a >= nt || term_b < 0 || term_b >= nt) return NEGF_EINVAL;
    pl->ta = ls->terms[term_a]; pl->tb = ls->terms[term_b];
    if (pl->ta->end == pl->tb->end) return NEGF_EINVAL;            // the corner blocks connect opposite end layers only
    pl->mirror = pl->tb->K < pl->ta->K;
    const RgfTerminal* s = pl->mirror ? pl->tb : pl->ta;
    pl->Ks = s->K; pl->Ko = (pl->mirror ? pl->ta : pl->tb)->K;
    if (pl->Ks > eig_wide_kmax()) return NEGF_EINVAL;
    pl->wide = c->channel_algo == 1 || pl->Ks > channels_kmax();
    pl->constant = s->kind == 0;
    *lsp = ls;
    return NEGF_OK;
}

int negf_layered_channel_count(negf_ctx* c, int h, int term_a, int term_b, int* nchan)
{
    if (!c || !nchan) return NEGF_EINVAL;
    LayeredSystem* ls; RgfChanPlan pl;
    if (int rc = rgf_chan_plan(c, h, term_a, term_b, &ls, &pl)) return rc;
    *nchan = pl.Ks;
    return NEGF_OK;
}

int negf_layered_transmission_channels_dev(negf_ctx* c, int h, int term_a, int term_b, int m, const double* E_dev, int nchan,
                                           double* T_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    RgfChanPlan pl;
    if ((rc = rgf_chan_plan(c, h, term_a, term_b, &ls, &pl))) return rc;
    if (nchan < 1 || !T_dev || (m > 0 && !E_dev)) return NEGF_EINVAL;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, false, &r))) return rc;
    RgfTerminal *ta = pl.ta, *tb = pl.tb;
    const int Ka = ta->K, Kb = tb->K, Ks = pl.Ks, Ko = pl.Ko;
    const size_t kk = (size_t)Ka * Kb, sa = (size_t)Ka * Ka, sb = (size_t)Kb * Kb, ks2 = (size_t)Ks * Ks, nbm = (size_t)r.nb_max;
    const size_t wide_per = pl.wide ? eig_wide_work_elems(Ks) : 0;
    const size_t per = sa + sb + 3 * kk + ks2 + wide_per, nl = pl.constant ? 1 : nbm, lstride = pl.constant ? 0 : ks2;
    if ((rc = ensure_cap(c, ls->d_chan, per * nbm + ks2 * nl)) || (rc = ensure_cap(c, ls->d_chan_rank, nl))) return rc;
    ls->work_bytes += 16LL * (long long)(per * nbm + ks2 * nl) + 4LL * (long long)nl;
    RgfCarve area{ls->d_chan.p};
    cplx *gamA = area.take(sa * nbm), *gamB = area.take(sb * nbm), *Gab = area.take(kk * nbm), *Z = area.take(kk * nbm);
    cplx *W = area.take(kk * nbm), *H = area.take(ks2 * nbm), *ework = area.take(wide_per * nbm), *Lh = area.take(ks2 * nl);
    int* rank = ls->d_chan_rank.p;
    // a on the last layer: G_ab is cut from G_{L-1,0}; a on layer 0: from G_{0,L-1} (as negf_layered_transmission_dev)
    const bool lower = ta->end == 1;
    const int ld = lower ? ls->n[0] : ls->n[ls->L - 1];
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) {
        cplx* Gc = nullptr;
        if (int e = rgf_corner_sweep(b, lower, &Gc)) return e;
        const cplx *sA, *sB; size_t stA, stB;
        rgf_sigma_of(ta, b.m0, &sA, &stA); rgf_sigma_of(tb, b.m0, &sB, &stB);
        {
            ProfScope ps(c, "gamma");
            launch_rgf_gamma(c->stream, Ka, b.nb, sA, stA, gamA, sa);
            launch_rgf_gamma(c->stream, Kb, b.nb, sB, stB, gamB, sb);
        }
        const cplx *gamS = pl.mirror ? gamB : gamA, *gamO = pl.mirror ? gamA : gamB;
        const size_t ss = pl.mirror ? sb : sa, so = pl.mirror ? sa : sb;
        if (!pl.constant || b.m0 == 0) {
            ProfScope ps(c, "eig");
            const int nf = pl.constant ? 1 : b.nb;
            const bool ok = pl.wide ? launch_pivoted_cholesky_wide(c->stream, Ks, nf, gamS, ss, Lh, ks2, rank)
                                    : launch_pivoted_cholesky(c->stream, Ks, nf, gamS, ss, Lh, ks2, rank);
            if (!ok) return NEGF_EINVAL;
        }
        {
            ProfScope ps(c, "zgemm");
            launch_gather_block(c->stream, ld, Ka, Kb, b.nb, Gc, ls->stride, ta->d_idx, tb->d_idx, Gab, kk);
            launch_zgemm(c->stream, Ks, Ko, Ks, b.nb, Lh, Ks, lstride, Gab, pl.mirror ? Ks : Ko, kk, pl.mirror ? 1 : 0, Z, Ko, kk);
            launch_zgemm(c->stream, Ks, Ko, Ko, b.nb, Z, Ko, kk, gamO, Ko, so, 0, W, Ko, kk);
            launch_zgemm(c->stream, Ks, Ks, Ko, b.nb, W, Ko, kk, Z, Ko, kk, 1, H, Ks, ks2);
        }
        ProfScope ps(c, "eig");
        // (all nchan columns are written: values, zeros beyond the rank or K_s, or a whole NaN row for a singular energy)
        double* Tb = T_dev + (size_t)b.m0 * nchan;
        const int rs = pl.constant ? 0 : 1;
        const bool ok = pl.wide ? launch_eigvalsh_wide(c->stream, Ks, b.nb, H, Ks, ks2, rank, rs, Tb, nchan, nchan, true, c->d_info + b.m0, true, -1, ework)
                                : launch_eigvalsh_batched(c->stream, Ks, b.nb, H, Ks, ks2, rank, rs, Tb, nchan, nchan, true, c->d_info + b.m0, true, -1);
        return ok ? NEGF_OK : NEGF_EINVAL;
    });
}

int negf_layered_transmission_channels(negf_ctx* c, int h, int term_a, int term_b, int m, const double* E, int nchan,
                                       double* T_chan, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    RgfChanPlan pl;
    if ((rc = rgf_chan_plan(c, h, term_a, term_b, &ls, &pl))) return rc;
    if (nchan < 1 || (m > 0 && (!E || !T_chan))) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    const size_t cnt = (size_t)m * nchan;
    if ((rc = stage_grid(c, m, 1, E, nullptr)) || (rc = ensure_cap(c, ls->d_chan_T, cnt))) return rc;
    if ((rc = negf_layered_transmission_channels_dev(c, h, term_a, term_b, m, dev_E(c), nchan, ls->d_chan_T))) return rc;
    ls->work_bytes += 8LL * (long long)cnt;
    return fetch_pageable(c, m, {{T_chan, ls->d_chan_T.p, cnt}}, info);
}

int negf_eigvalsh_wide_batched(negf_ctx* c, int K, int m, const double* A, double* w, int* info)
{
    if (!c) return NEGF_EINVAL;
    if (K < 1 || K > eig_wide_kmax() || m < 0 || (m > 0 && (!A || !w))) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    const size_t k2 = (size_t)K * K;
    cplx *dA = nullptr, *dwork = nullptr; double* dw = nullptr; int* di = nullptr;
    std::vector<int> hi((size_t)m);
    // (one way out: whatever fails, everything allocated so far is freed below)
    int rc = dev_alloc(&dA, k2 * m);
    if (!rc) rc = dev_alloc(&dwork, eig_wide_work_elems(K) * m);
    if (!rc) rc = dev_alloc(&dw, (size_t)K * m);
    if (!rc) rc = dev_alloc(&di, (size_t)m);
    if (!rc) rc = upload(c, dA, reinterpret_cast<const cplx*>(A), k2 * m);
    if (!rc) {
        ProfScope ps(c, "eig");
        if (!launch_eigvalsh_wide(c->stream, K, m, dA, K, k2, nullptr, 0, dw, K, K, false, di, false, 1, dwork)) rc = NEGF_EINVAL;
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = NEGF_EHIP;
    if (!rc) rc = download(c, w, dw, (size_t)K * m);
    if (!rc) rc = download(c, hi.data(), di, (size_t)m);
    dev_free(dA); dev_free(dwork); dev_free(dw); dev_free(di);
    if (rc) return rc;
    for (int i = 0; i < m; ++i) {
        if (info) info[i] = hi[i];
        if (hi[i] != 0) rc = NEGF_ESINGULAR;
    }
    return rc;
}

int negf_set_channel_algo(negf_ctx* c, int algo)
{
    if (!c || (algo != 0 && algo != 1)) return NEGF_EINVAL;
    c->channel_algo = algo;
    return NEGF_OK;
}

// negf_layered_dos_dev (ind null) and negf_layered_contact_dos_dev
static int rgf_dev_dos(negf_ctx* c, int h, int form, const int* ind, int m, const double* E_dev, double* dos_total_dev, double* dos_site_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if ((form != 0 && form != 1) || (m > 0 && (!E_dev || !dos_total_dev || !dos_site_dev))) return NEGF_EINVAL;
    RgfLess less;
    if (ind && (rc = rgf_less_select(c, ls, *ind, &less))) return rc;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, less.per_energy))) return rc;
    if (ind) rgf_less_layout(r, &less);
    const RgfDosBlocks dos{form, dos_site_dev};
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) {
        if (int e = rgf_pattern_batch(b, ind ? &less : nullptr, dos)) return e;
        ProfScope ps(c, "rgf");
        launch_rgf_dos_total(c->stream, ls->N, b.nb, dos_site_dev + (size_t)b.m0 * ls->N, (size_t)ls->N, dos_total_dev + b.m0);
        return NEGF_OK;
    });
}

int negf_layered_dos_dev(negf_ctx* c, int h, int form, int m, const double* E_dev, double* dos_total_dev, double* dos_site_dev)
{
    return rgf_dev_dos(c, h, form, nullptr, m, E_dev, dos_total_dev, dos_site_dev);
}

int negf_layered_contact_dos_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, double* dos_total_dev, double* dos_site_dev)
{
    return rgf_dev_dos(c, h, 1, &ind, m, E_dev, dos_total_dev, dos_site_dev);
}

// negf_layered_gr_int_dev (ind null) and negf_layered_gless_int_dev
static int rgf_dev_pattern_int(negf_ctx* c, int h, const int* ind, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    RgfLess less;
    if (ind && (rc = rgf_less_select(c, ls, *ind, &less))) return rc;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, less.per_energy))) return rc;
    if (ind) rgf_less_layout(r, &less);
    const RgfSumBlocks sum{reinterpret_cast<const cplx*>(w_dev), reinterpret_cast<cplx*>(out_dev)};
    NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, (ls->dtot + 2 * ls->utot) * sizeof(cplx), c->stream));
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) { return rgf_pattern_batch(b, ind ? &less : nullptr, sum); });
}

int negf_layered_gr_int_dev(negf_ctx* c, int h, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    return rgf_dev_pattern_int(c, h, nullptr, m, E_dev, w_dev, out_dev);
}

int negf_layered_gless_int_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    return rgf_dev_pattern_int(c, h, &ind, m, E_dev, w_dev, out_dev);
}

static int rgf_host_pattern_int(negf_ctx* c, int h, const int* ind, int m, const double* E, const double* w, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    if (ind && !rgf_less_ind_ok(ls, *ind)) return NEGF_EINVAL;
    const size_t tot = ls->dtot + 2 * ls->utot;
    if ((rc = stage_grid(c, m, 1, E, w, tot * sizeof(cplx))) || (rc = ensure_cap(c, ls->d_out, tot))) return rc;
    if ((rc = rgf_dev_pattern_int(c, h, ind, m, dev_E(c), dev_w(c), reinterpret_cast<double*>(ls->d_out.p)))) return rc;
    return fetch_result_and_info(c, m, ls->d_out.p, tot * sizeof(cplx), out, info);
}

int negf_layered_gr_int(negf_ctx* c, int h, int m, const double* E, const double* w, double* out, int* info)
{
    return rgf_host_pattern_int(c, h, nullptr, m, E, w, out, info);
}

int negf_layered_gless_int(negf_ctx* c, int h, int ind, int m, const double* E, const double* w, double* out, int* info)
{
    return rgf_host_pattern_int(c, h, &ind, m, E, w, out, info);
}

// negf_layered_dos (form, ind null) and negf_layered_contact_dos: grid staged, totals and per-site rows fetched
static int rgf_host_dos(negf_ctx* c, int h, int form, const int* ind, int m, const double* E, double* dos_total, double* dos_site, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if ((form != 0 && form != 1) || (m > 0 && (!E || !dos_total))) return NEGF_EINVAL;
    if (ind && !rgf_less_ind_ok(ls, *ind)) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    if ((rc = stage_grid(c, m, 1, E, nullptr)) || (rc = ensure_cap(c, ls->d_site, (size_t)m * ls->N))) return rc;
    if ((rc = rgf_dev_dos(c, h, form, ind, m, dev_E(c), c->d_scal, ls->d_site))) return rc;
    return fetch_pageable(c, m, {{dos_site, ls->d_site.p, dos_site ? (size_t)m * ls->N : 0}, {dos_total, c->d_scal, (size_t)m}}, info);
}

int negf_layered_dos(negf_ctx* c, int h, int form, int m, const double* E, double* dos_total, double* dos_site, int* info)
{
    return rgf_host_dos(c, h, form, nullptr, m, E, dos_total, dos_site, info);
}

int negf_layered_contact_dos(negf_ctx* c, int h, int ind, int m, const double* E, double* dos_total, double* dos_site, int* info)
{
    return rgf_host_dos(c, h, 1, &ind, m, E, dos_total, dos_site, info);
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
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, pl.per_energy))) return rc;
    ls->work_bytes += 16LL * (long long)pl.stat;
    if ((rc = rgf_tmat_setup(c, ls, psig, &pl))) return rc;
    const size_t C2 = (size_t)pl.C * pl.C;
    RgfCarve cols{ls->d_cols.p};
    rgf_tmat_layout(r, &pl, &cols);
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) { return rgf_tmat_batch(b, pl, T_dev + C2 * b.m0); });
}

int negf_layered_transmission_matrix(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                     const double* probe_sigma, int m, const double* E, double* T, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    const long Cl = (long)ls->terms.size() + n_probes;
    if (n_probes < 0 || Cl < 1 || Cl > TMAT_MAX_TERMINALS || (m > 0 && (!E || !T))) return NEGF_EINVAL;
    const size_t C = ls->terms.size() + (size_t)n_probes, cnt = (size_t)m * C * C;
    if ((rc = stage_grid(c, m, 1, E, nullptr)) || (rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_layered_transmission_matrix_dev(c, h, n_probes, probe_nk, probe_inds, probe_sigma, m,
                                                   dev_E(c), c->d_bond_T))) return rc;
    return fetch_pageable(c, m, {{T, c->d_bond_T.p, cnt}}, info);
}

// ------------------------------------------------- floating probes on layers: response, G^<, G^r
// The probes of negf_layered_transmission_matrix left floating at every energy, as negf_probe_response,
// negf_gless_int_probes and negf_gr_int_probes leave the dense system's: nothing crosses to the host.
int negf_layered_probe_response_dev(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                    const double* probe_sigma, int m, const double* E_dev, double* R_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    RgfTmatPlan pl;
    const cplx* psig = reinterpret_cast<const cplx*>(probe_sigma);
    if ((rc = rgf_tmat_plan(ls, n_probes, probe_nk, probe_inds, psig, &pl))) return rc;
    if (m > 0 && (!E_dev || (n_probes > 0 && !R_dev))) return NEGF_EINVAL;
    if (m == 0) { c->last_m = 0; return NEGF_OK; }
    // a transmission-matrix call whose matrices stay in a per-batch area, the response kernel behind each batch
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, pl.per_energy))) return rc;
    const size_t C2 = (size_t)pl.C * pl.C, pc = (size_t)n_probes * pl.nt;
    ls->work_bytes += 16LL * (long long)pl.stat + 8LL * (long long)C2 * r.nb_max;
    if ((rc = rgf_tmat_setup(c, ls, psig, &pl)) || (rc = ensure_cap(c, ls->d_deph_T, C2 * r.nb_max))) return rc;
    RgfCarve cols{ls->d_cols.p};
    rgf_tmat_layout(r, &pl, &cols);
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) {
        if (int e = rgf_tmat_batch(b, pl, ls->d_deph_T)) return e;
        return deph_run_response(c, pl.C, pl.nt, pl.d_porder, b.nb, ls->d_deph_T, R_dev + pc * b.m0);
    });
}

int negf_layered_probe_response(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                const double* probe_sigma, int m, const double* E, double* R, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    const long Cl = (long)ls->terms.size() + n_probes;
    if (n_probes < 0 || Cl < 1 || Cl > TMAT_MAX_TERMINALS || (m > 0 && (!E || (n_probes > 0 && !R)))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * n_probes * ls->terms.size();
    if ((rc = stage_grid(c, m, 1, E, nullptr)) || (rc = ensure_cap(c, ls->d_deph_out, cnt + 1))) return rc;
    if ((rc = negf_layered_probe_response_dev(c, h, n_probes, probe_nk, probe_inds, probe_sigma, m, dev_E(c), ls->d_deph_out))) return rc;
    if (cnt == 0) return fetch_pageable(c, m, {}, info);
    return fetch_pageable(c, m, {{R, ls->d_deph_out.p, cnt}}, info);
}

int negf_layered_gless_int_probes_dev(negf_ctx* c, int h, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                                      const double* probe_sigma, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!rgf_less_ind_ok(ls, ind)) return NEGF_EINVAL;
    RgfTmatPlan pl;
    const cplx* psig = reinterpret_cast<const cplx*>(probe_sigma);
    if ((rc = rgf_tmat_plan(ls, n_probes, probe_nk, probe_inds, psig, &pl))) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    RgfDephPlan dp;
    if ((rc = rgf_deph_plan(ls, pl, ind, &dp))) return rc;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, dp.per_energy))) return rc;
    ls->work_bytes += 16LL * (long long)pl.stat;
    if (dp.floating) ls->work_bytes += 8LL * (long long)((size_t)pl.C * pl.C + (size_t)n_probes * pl.nt) * r.nb_max;
    if ((rc = rgf_tmat_setup(c, ls, psig, &pl)) || (rc = rgf_deph_setup(c, ls, pl, r, &dp))) return rc;
    const size_t nbm = (size_t)r.nb_max;
    RgfCarve cols{ls->d_cols.p};
    dp.keep = cols.take((size_t)ls->L * pl.cs * nbm); dp.Y = cols.take((size_t)ls->L * pl.cs * nbm);
    pl.gdyn = cols.take(pl.dyn * nbm);
    pl.Gab = cols.take(pl.big_kk * nbm); pl.Xs = cols.take(pl.big_kk * nbm); pl.Ys = cols.take(pl.big_kk * nbm);
    dp.D = cols.take(dp.Dtot * nbm);
    const RgfSumBlocks sum{reinterpret_cast<const cplx*>(w_dev), reinterpret_cast<cplx*>(out_dev)};
    NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, (ls->dtot + 2 * ls->utot) * sizeof(cplx), c->stream));
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) { return rgf_deph_batch(b, pl, dp, sum); });
}

// sum_k w_k G(E_k) on the pattern with the probes in A: negf_layered_gr_int_dev's two sweeps with the probes of each layer
// taken out of its diagonal before the inverse, as the transmission matrix's factor sweep takes them
int negf_layered_gr_int_probes_dev(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                                   const double* probe_sigma, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    RgfTmatPlan pl;
    const cplx* psig = reinterpret_cast<const cplx*>(probe_sigma);
    if ((rc = rgf_tmat_plan(ls, n_probes, probe_nk, probe_inds, psig, &pl))) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r))) return rc;
    ls->work_bytes += 16LL * (long long)pl.stat;
    if ((rc = rgf_tmat_setup(c, ls, psig, &pl))) return rc;
    const RgfSumBlocks sum{reinterpret_cast<const cplx*>(w_dev), reinterpret_cast<cplx*>(out_dev)};
    NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, (ls->dtot + 2 * ls->utot) * sizeof(cplx), c->stream));
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) {
        const RgfView v{ls, false};
        const int e = rgf_factor_sweep(b, v, rgf_sub_probes_step(b, v, pl), rgf_no_step);
        return e ? e : rgf_solve_sweep(b, v, sum);
    });
}

// the host forms of the two sums: grid and weights staged, the block lists and the info back through the pinned buffer
static int rgf_host_probes_int(negf_ctx* c, int h, const int* ind, int n_probes, const int* probe_nk, const int* probe_inds,
                               const double* probe_sigma, int m, const double* E, const double* w, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    const long Cl = (long)ls->terms.size() + n_probes;
    if (n_probes < 0 || Cl < 1 || Cl > TMAT_MAX_TERMINALS || !out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    if (ind && !rgf_less_ind_ok(ls, *ind)) return NEGF_EINVAL;
    const size_t tot = ls->dtot + 2 * ls->utot;
    if ((rc = stage_grid(c, m, 1, E, w, tot * sizeof(cplx))) || (rc = ensure_cap(c, ls->d_out, tot))) return rc;
    double* acc = reinterpret_cast<double*>(ls->d_out.p);
    rc = ind ? negf_layered_gless_int_probes_dev(c, h, *ind, n_probes, probe_nk, probe_inds, probe_sigma, m, dev_E(c), dev_w(c), acc)
             : negf_layered_gr_int_probes_dev(c, h, n_probes, probe_nk, probe_inds, probe_sigma, m, dev_E(c), dev_w(c), acc);
    if (rc) return rc;
    return fetch_result_and_info(c, m, ls->d_out.p, tot * sizeof(cplx), out, info);
}

int negf_layered_gless_int_probes(negf_ctx* c, int h, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                                  const double* probe_sigma, int m, const double* E, const double* w, double* out, int* info)
{
    return rgf_host_probes_int(c, h, &ind, n_probes, probe_nk, probe_inds, probe_sigma, m, E, w, out, info);
}

int negf_layered_gr_int_probes(negf_ctx* c, int h, int n_probes, const int* probe_nk, const int* probe_inds,
                               const double* probe_sigma, int m, const double* E, const double* w, double* out, int* info)
{
    return rgf_host_probes_int(c, h, nullptr, n_probes, probe_nk, probe_inds, probe_sigma, m, E, w, out, info);
}

// negf_layered_local_transmission_dev (w null, per-energy tables) and negf_layered_bond_int_dev: negf_local_transmission_dev
// and negf_bond_int_dev on a layered system -- the G Gamma G^H call of rgf_dev_pattern_int with RgfBondBlocks as its sink
static int rgf_dev_bond(negf_ctx* c, int h, int ind, int m, const double* E_dev, const double* w_dev, bool integral,
                        const int* groups_per_layer, const int* group_of, double* out_dev)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!rgf_less_ind_ok(ls, ind)) return NEGF_EINVAL;
    if (integral ? (!out_dev || (m > 0 && (!E_dev || !w_dev))) : (m > 0 && (!E_dev || !out_dev))) return NEGF_EINVAL;
    RgfBondGroups bg;
    if ((rc = rgf_bond_groups(ls, groups_per_layer, group_of, &bg))) return rc;
    RgfLess less;
    if ((rc = rgf_less_select(c, ls, ind, &less))) return rc;
    RgfRun r;
    if ((rc = ensure_mbuffers(c, m, 1)) || (rc = rgf_workspace(c, ls, m, true, &r, less.per_energy))) return rc;
    rgf_less_layout(r, &less);
    if (bg.mapped) {
        if ((rc = ensure_cap(c, ls->d_bond_map, bg.map.size())) || (rc = upload(c, ls->d_bond_map.p, bg.map.data(), bg.map.size()))) return rc;
        bg.d_map = ls->d_bond_map;
        ls->work_bytes += (long long)(bg.map.size() * sizeof(int));
    }
    if (integral) NEGF_HIP_CHECK(hipMemsetAsync(out_dev, 0, bg.table() * sizeof(double), c->stream));
    const RgfBondBlocks bond{integral ? w_dev : nullptr, out_dev, &bg};
    return rgf_batches(r, m, E_dev, [&](const RgfBatch& b) { return rgf_less_batch(b, &less, bond); });
}

int negf_layered_local_transmission_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, const int* groups_per_layer,
                                        const int* group_of, double* out_dev)
{
    return rgf_dev_bond(c, h, ind, m, E_dev, nullptr, false, groups_per_layer, group_of, out_dev);
}

int negf_layered_bond_int_dev(negf_ctx* c, int h, int ind, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    return rgf_dev_bond(c, h, ind, m, E_dev, w_dev, true, nullptr, nullptr, out_dev);
}

int negf_layered_local_transmission(negf_ctx* c, int h, int ind, int m, const double* E, const int* groups_per_layer,
                                    const int* group_of, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!rgf_less_ind_ok(ls, ind) || (m > 0 && (!E || !out))) return NEGF_EINVAL;
    RgfBondGroups bg;
    if ((rc = rgf_bond_groups(ls, groups_per_layer, group_of, &bg))) return rc;
    if (m == 0) return NEGF_OK;
    const size_t cnt = (size_t)m * bg.table();
    if ((rc = stage_grid(c, m, 1, E, nullptr)) || (rc = ensure_cap(c, ls->d_bond_out, cnt))) return rc;
    if ((rc = rgf_dev_bond(c, h, ind, m, dev_E(c), nullptr, false, groups_per_layer, group_of, ls->d_bond_out))) return rc;
    ls->work_bytes += (long long)(cnt * sizeof(double));
    return fetch_pageable(c, m, {{out, ls->d_bond_out.p, cnt}}, info);
}

int negf_layered_bond_int(negf_ctx* c, int h, int ind, int m, const double* E, const double* w, double* out, int* info)
{
    LayeredSystem* ls;
    int rc = rgf_open(c, h, m, &ls);
    if (rc) return rc;
    if (!rgf_less_ind_ok(ls, ind) || !out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    const size_t tot = ls->dtot + 2 * ls->utot, ob = tot * sizeof(double);
    if ((rc = stage_grid(c, m, 1, E, nullptr, ob)) || (rc = stage_real_weights(c, m, w, ob)) || (rc = ensure_cap(c, ls->d_bond_out, tot))) return rc;
    if ((rc = rgf_dev_bond(c, h, ind, m, dev_E(c), dev_w(c), true, nullptr, nullptr, ls->d_bond_out))) return rc;
    ls->work_bytes += (long long)ob;
    return fetch_result_and_info(c, m, ls->d_bond_out.p, ob, out, info);
}

int negf_layered_workspace_bytes(negf_ctx* c, int h, long long* work)
{
    LayeredSystem* ls = get_layered(c, h);
    if (!ls || !work) return NEGF_EINVAL;
    *work = ls->work_bytes;
    return NEGF_OK;
}

}  // extern "C"
