// C ABI of libnegf_hip.so (include/negf.h): context, self-energy providers and the
// orchestration of the per-batch kernel sequence.  No compute happens on the
// host here; there is no CPU fallback (negf_create fails without a GPU).
#include "negf_common.h"
#include <algorithm>
#include <atomic>
#include <thread>
#include <cstdlib>
#include <initializer_list>
#include <new>

static hipEvent_t prof_get_event(negf_ctx* c)
{
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

FlopCount g_negf_flops;

ProfScope::ProfScope(negf_ctx* ctx, const char* nm) : c(ctx), name(nm)
{
    if (!c->profiling) return;
    f0 = g_negf_flops;
    e0 = prof_get_event(c); e1 = prof_get_event(c);
    if (e0) (void)hipEventRecord(e0, c->stream);
}

ProfScope::~ProfScope()
{
    if (!c->profiling) return;
    { auto& e = c->prof[name]; e.flops_alg += g_negf_flops.alg - f0.alg; e.flops_mfma += g_negf_flops.mfma - f0.mfma; }
    if (!e0 || !e1) return;
    (void)hipEventRecord(e1, c->stream);
    c->prof_pending.push_back({name, e0, e1});
}

static void prof_resolve(negf_ctx* c)
{
    for (auto& p : c->prof_pending) {
        (void)hipEventSynchronize(p.e1);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            auto& e = c->prof[p.name]; e.ms += ms; e.launches += 1;
        }
        c->ev_pool.push_back(p.e0); c->ev_pool.push_back(p.e1);
    }
    c->prof_pending.clear();
}

namespace {

int wait_stream(negf_ctx* c);

// every live context of the process: when an allocation fails, the g(E) caches (up to 8 GB each, reusable results, not
// state) are dropped before the allocation is given up
std::vector<negf_ctx*>& live_contexts() { static std::vector<negf_ctx*> v; return v; }
bool drop_gcaches();

template <typename T>
int dev_alloc(T** p, size_t count, bool may_drop_caches = true /* false: the allocation IS a cache entry */)
{
    *p = nullptr;
    if (count == 0) return NEGF_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (may_drop_caches && drop_gcaches()) e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));      // once more without the caches
        if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return NEGF_ENOMEM; }
    }
    return NEGF_OK;
}
template <typename T>
void dev_free(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

// Grow-only device buffers (DevBuf): nothing happens while the buffer holds `need` elements; otherwise the context's
// stream is drained first (queued work may still read the old buffer), the buffer freed and a new one allocated.
template <typename T>
int ensure_cap(negf_ctx* c, DevBuf<T>& b, size_t need)
{
    if (need <= b.cap) return NEGF_OK;
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    dev_free(b.p); b.cap = 0;
    int rc = dev_alloc(&b.p, need);
    if (rc) return rc;
    b.cap = need;
    return NEGF_OK;
}
template <typename... B>
void release_bufs(B&... b) { ((dev_free(b.p), b.cap = 0), ...); }

template <typename T>
int upload(negf_ctx* c, T* dst, const T* src, size_t count)
{
    if (count == 0) return NEGF_OK;
    NEGF_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));   // src may be freed by the caller on return
    return NEGF_OK;
}
template <typename T>
int download(negf_ctx* c, T* dst, const T* src, size_t count)
{
    if (count == 0) return NEGF_OK;
    NEGF_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return wait_stream(c);
}

void free_provider(SigmaProvider* p)
{
    if (!p) return;
    dev_free(p->d_const_c); dev_free(p->d_const_tot); dev_free(p->d_hbase); dev_free(p->d_const_blk);
    dev_free(p->d_inds); dev_free(p->d_nc); dev_free(p->d_blk_off); dev_free(p->d_inds_off);
    dev_free(p->d_n_atoms); dev_free(p->d_atom_off); dev_free(p->d_pos);
    dev_free(p->d_alpha); dev_free(p->d_Salpha); dev_free(p->d_beta); dev_free(p->d_Sbeta);
    dev_free(p->d_tau); dev_free(p->d_Stau); dev_free(p->d_lead_pad);
    dev_free(p->d_atom_orbs); dev_free(p->d_nb_off); dev_free(p->d_nb_dirs);
    dev_free(p->d_H); dev_free(p->d_Slist); dev_free(p->d_Vlist); dev_free(p->d_xi);
    dev_free(p->d_pre_tot); dev_free(p->d_pre_c); release_bufs(p->d_order); dev_free(p->d_prevE); dev_free(p->d_prev_iters); dev_free(p->d_curE); dev_free(p->d_cur_iters);
    delete p;
}

// the work areas sized by the batch, and the grow-only buffers that scale with it (all of the latter: all = true)
void free_workspace(negf_ctx* c, bool all = false)
{
    dev_free(c->d_A); dev_free(c->d_T1); dev_free(c->d_T2); dev_free(c->d_ipiv); dev_free(c->d_site);
    c->batch = 0;
    release_bufs(c->d_blk, c->d_scratch, c->d_gsmall, c->d_small_part);
    if (all) release_bufs(c->d_seg_out, c->d_ref_P, c->d_chan, c->d_chan_rank, c->d_chan_T, c->d_chan_psi, c->d_bond_map, c->d_bond_carry, c->d_bond_T, c->d_pop_W, c->d_pop_Wt,
                          c->d_tmat_H, c->d_tmat_sig, c->d_tmat_gam, c->d_tmat_work, c->d_tmat_tab,
                          c->d_deph_T, c->d_deph_R, c->d_deph_work, c->d_deph_D, c->d_deph_carry, c->d_deph_tab);
}

void free_mbuffers(negf_ctx* c)
{
    dev_free(c->d_info); dev_free(c->d_iters); dev_free(c->d_conv);
    dev_free(c->d_E); dev_free(c->d_w); dev_free(c->d_scal);
    c->m_cap = 0; c->contacts_cap = 0; c->h_E_valid = false;
}

void free_gentry(ChainGEntry& e)
{
    dev_free(e.d_g); dev_free(e.d_it); dev_free(e.d_cv);
    e.g_cap = 0; e.it_cap = 0; e.valid = false;
}

void free_gcache(negf_ctx* c)
{
    for (auto& e : c->gcache) free_gentry(e);
    c->gcache.clear();
}

// true: something was freed.  (Entries in use by a launch in flight are freed by hipFree after that launch: hipFree
// synchronises the device.)
bool drop_gcaches()
{
    bool any = false;
    for (negf_ctx* c : live_contexts())
        if (!c->gcache.empty() && !c->gcache_pinned) { free_gcache(c); any = true; }
    return any;
}

// 64-bit mixing hash over the 8-byte words of a buffer (a filter in front of the bitwise comparisons of the g(E) cache)
unsigned long long hash_words(const void* data, size_t bytes, unsigned long long h = 0x9E3779B97F4A7C15ull)
{
    const unsigned long long* w = static_cast<const unsigned long long*>(data);
    for (size_t i = 0; i < bytes / 8; ++i) { h = (h ^ w[i]) * 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    return h;
}

// the energies E_dev[0..nb) on the host: the copy stage_grid kept when they are the staged grid, a download otherwise
const cplx* host_energies(negf_ctx* c, const cplx* E_dev, int nb, std::vector<cplx>& tmp)
{
    if (c->h_E_valid && c->d_E && E_dev >= c->d_E && E_dev + nb <= c->d_E + c->h_E.size())
        return c->h_E.data() + (E_dev - c->d_E);
    tmp.resize((size_t)nb);
    if (hipMemcpyAsync(tmp.data(), E_dev, (size_t)nb * sizeof(cplx), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return tmp.data();
}

// Look the launch (provider p, energies Eh[0..nb)) up in the context's g(E) cache.  *hit: the entry holds it.  Otherwise
// the returned entry (least recently used, or a new one) has room for it and is to be filled by the launch; nullptr:
// not cached (cache off, entry too large, out of memory).
ChainGEntry* gcache_lookup(negf_ctx* c, const SigmaProvider* p, const cplx* Eh, int nb, bool* hit)
{
    *hit = false;
    if (c->gcache_max <= 0 || !Eh || nb <= 0 || !p->h_lead) return nullptr;
    const size_t g_elems = (size_t)nb * p->blk_stride, it_elems = (size_t)nb * p->n_contacts;
    if (g_elems * sizeof(cplx) > c->gcache_entry_bytes_max) return nullptr;
    const unsigned long long eh = hash_words(Eh, (size_t)nb * sizeof(cplx));
    for (auto& e : c->gcache) {
        if (!e.valid || e.E_hash != eh || e.lead_hash != p->lead_hash || (int)e.E.size() != nb) continue;
        if (e.eta != p->eta || e.conv != p->conv || e.relFactor != p->relFactor || e.max_iter != p->max_iter ||
            e.force_iters != p->force_iters || e.solver != p->solver || e.nc != p->nc) continue;
        if (std::memcmp(e.E.data(), Eh, (size_t)nb * sizeof(cplx)) != 0) continue;
        if (e.lead != p->h_lead && (e.lead->size() != p->h_lead->size() ||
                                    std::memcmp(e.lead->data(), p->h_lead->data(), e.lead->size() * sizeof(cplx)) != 0)) continue;
        e.used = ++c->gcache_clock;
        ++c->gcache_hits;
        *hit = true;
        return &e;
    }
    ++c->gcache_misses;
    // room for the new entry: a free slot while the cache is below its entry and byte limits, else the least
    // recently used entries go -- one whose buffers are large enough is reused as it is
    auto bytes_of = [](const ChainGEntry& e) { return e.g_cap * sizeof(cplx) + 2 * e.it_cap * sizeof(int); };
    const size_t need_b = g_elems * sizeof(cplx) + 2 * it_elems * sizeof(int);
    size_t held = 0;
    for (const auto& e : c->gcache) held += bytes_of(e);
    ChainGEntry* v = nullptr;
    for (auto& e : c->gcache) if (!e.valid && e.g_cap >= g_elems && e.it_cap >= it_elems) { v = &e; break; }   // an invalidated entry that fits
    bool synced = false;
    while (!v) {
        int with_buffers = 0;
        ChainGEntry *lru = nullptr, *empty = nullptr;
        for (auto& e : c->gcache) {
            if (!e.d_g) { if (!empty) empty = &e; continue; }
            ++with_buffers;
            if (!lru || (!e.valid && lru->valid) || (e.valid == lru->valid && e.used < lru->used)) lru = &e;
        }
        if (with_buffers < c->gcache_max && held + need_b <= c->gcache_bytes_max) {
            if (!empty) { c->gcache.emplace_back(); empty = &c->gcache.back(); }     // (capacity reserved: no reallocation)
            v = empty;
            break;
        }
        if (!lru) return nullptr;                                                    // larger than the whole budget
        lru->valid = false;
        if (lru->g_cap >= g_elems && lru->it_cap >= it_elems) { v = lru; break; }    // taken over as it is
        if (!synced) { (void)hipStreamSynchronize(c->stream); synced = true; }       // earlier kernels may still read it
        held -= bytes_of(*lru);
        free_gentry(*lru);
    }
    if (g_elems > v->g_cap || it_elems > v->it_cap) {
        free_gentry(*v);
        if (dev_alloc(&v->d_g, g_elems, false) || dev_alloc(&v->d_it, it_elems, false) || dev_alloc(&v->d_cv, it_elems, false)) { free_gentry(*v); return nullptr; }
        v->g_cap = g_elems; v->it_cap = it_elems;
    }
    v->nc = p->nc; v->lead = p->h_lead; v->lead_hash = p->lead_hash; v->E_hash = eh;
    v->eta = p->eta; v->conv = p->conv; v->relFactor = p->relFactor; v->max_iter = p->max_iter; v->force_iters = p->force_iters;
    v->solver = p->solver;
    v->E.assign(Eh, Eh + nb);
    v->used = ++c->gcache_clock;
    return v;
}

// Energies in flight for a grid of m points.  Once the transmission entry point has been used on this context
// the workspace is sized for TWICE the grid (it carves two work areas per energy out of it), so that the calls of
// one workflow -- GrInt, calculate_transmission, GrLessInt on the same grid -- find it in place: it only ever
// grows, and only when a larger grid arrives.  Contexts that only integrate (SCF loops, the headline bench) get
// the single-grid size: half the HBM, which matters when ranks or processes share a device.
int auto_batch(negf_ctx* c, int m)
{
    if (c->batch_user > 0) return std::min(c->batch_user, std::max(m, 1));
    m = (c->transmission_seen ? 2 : 1) * std::max(m, 1);
    // three n x n complex128 work matrices per in-flight energy.  The working set may take a
    // quarter of the free HBM (288 GB per MI355X), at most 64 GB: large matrices need hundreds of
    // energies in flight so that the one-workgroup-per-matrix panel kernels cover the 256 CUs
    // (n = 2000: 192 MB per energy -> 333 in flight); never above the grid length.
    const double per = 3.0 * 16.0 * (double)c->n * (double)c->n;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)24e9;
    const double budget = std::min(64.0e9, std::max(2.0e9, 0.25 * (double)free_b));
    long b = (long)(budget / std::max(per, 1.0));
    b = std::max(1L, std::min(b, 4096L));
    return (int)std::min<long>(b, std::max(m, 1));
}

int ensure_workspace(negf_ctx* c, int m, int blk_stride, int min_batch = 1)
{
    // (the workspace in place already covers the grid: no hipMemGetInfo, which costs more than a small integral)
    const int covers = (c->transmission_seen ? 2 : 1) * std::max(m, 1);
    const int want = (c->batch_user == 0 && c->batch >= std::min(covers, 4096) && c->batch >= min_batch)
                         ? c->batch : std::max(auto_batch(c, m), min_batch);
    // (a limit set with negf_set_batch holds for a workspace already in place: one larger than the limit -- and than the two
    //  energies a transmission call needs -- is released and rebuilt at `want`; no dense call sweeps more than the limit)
    const bool over_limit = c->batch_user > 0 && c->batch > std::max(c->batch_user, min_batch);
    if (want > c->batch || over_limit) {
        free_workspace(c);
        const size_t n2 = (size_t)c->n * c->n;
        int rc;
        // (+ 64 elements: a guard behind the last matrix; no kernel relies on it any more -- the column-block
        //  update of the windowed inverse clamps its lane offset to the window width)
        if ((rc = dev_alloc(&c->d_A, n2 * want + 64))) return rc;
        if ((rc = dev_alloc(&c->d_T1, n2 * want + 64))) return rc;
        if ((rc = dev_alloc(&c->d_T2, n2 * want + 64))) return rc;
        if ((rc = dev_alloc(&c->d_ipiv, (size_t)2 * c->n * want))) return rc;
        if ((rc = dev_alloc(&c->d_site, (size_t)c->n * want))) return rc;
        c->batch = want;
    }
    return ensure_cap(c, c->d_blk, (size_t)blk_stride * c->batch);
}

// Wait for the context's stream at the end of a host-pointer call.  hipStreamSynchronize parks the thread and is woken
// by an interrupt -- tens of microseconds after the GPU is done, as much as a small integral itself takes -- so the
// stream is POLLED for the first 2 ms (an SCF-sized call is over long before) and only then handed to the blocking wait.
int wait_stream(negf_ctx* c)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return NEGF_OK;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return NEGF_OK;
}

void free_pinned(negf_ctx* c)
{
    if (c->h_pin) { (void)hipHostFree(c->h_pin); c->h_pin = nullptr; c->h_pin_cap = 0; }
    if (c->gj_side.ok) {
        (void)hipEventDestroy(c->gj_side.fork);
        for (int g = 0; g < GjSideStreams::MAXG - 1; ++g) { (void)hipStreamDestroy(c->gj_side.s[g]); (void)hipEventDestroy(c->gj_side.join[g]); }
        c->gj_side.ok = false;
    }
}

int ensure_pinned(negf_ctx* c, size_t bytes)
{
    if (bytes <= c->h_pin_cap) return NEGF_OK;
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));           // copies from / into the old buffer
    free_pinned(c);
    const size_t cap = std::max(bytes + bytes / 2, (size_t)1 << 20);
    void* q = nullptr;
    if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return NEGF_ENOMEM; }
    c->h_pin = static_cast<unsigned char*>(q); c->h_pin_cap = cap;
    return NEGF_OK;
}

// ---- small systems: the single-kernel path (k_small_fused.hip)
bool small_path(const negf_ctx* c, const SigmaProvider* p)
{
    if (c->small_algo != 0 || c->inverse_algo != 0 || !small_fused_supported(c->n)) return false;
    if (p->kind == SK_CONST || p->kind == SK_PRECOMPUTED) return true;
    return (p->kind == SK_CHAIN1D || p->kind == SK_BETHE) && !p->d_xi && p->d_pos;
}

// arguments of the fused kernel for the energies [m0, m0 + nb) of provider p (Sigma blocks of a block provider are in
// c->d_blk: run_sigma_blocks has run for exactly this range)
SmallFusedArgs small_args(negf_ctx* c, SigmaProvider* p, int m0, int nb, const cplx* E)
{
    SmallFusedArgs a;
    a.n = c->n; a.m = nb; a.E = E + m0; a.S = c->d_S; a.H = c->d_F;
    a.info = c->d_info + m0;
    const size_t n2 = (size_t)c->n * c->n;
    if (p->kind == SK_CONST) a.H = p->d_hbase;
    else if (p->kind == SK_PRECOMPUTED) { a.sig_dense = p->d_pre_tot + n2 * m0; a.sig_stride = n2; }
    else { a.blk = c->d_blk; a.blk_stride = p->blk_stride; a.n_contacts = p->n_contacts; a.pos = p->d_pos; a.nc = p->d_nc; a.blk_off = p->d_blk_off; }
    return a;
}

int ensure_mbuffers(negf_ctx* c, int m, int contacts)
{
    contacts = std::max(contacts, 1);
    if (m <= c->m_cap && contacts <= c->contacts_cap) return NEGF_OK;
    const int mm = std::max(m, c->m_cap), cc = std::max(contacts, c->contacts_cap);
    free_mbuffers(c);
    int rc;
    if ((rc = dev_alloc(&c->d_info, (size_t)mm))) return rc;
    if ((rc = dev_alloc(&c->d_iters, (size_t)mm * cc))) return rc;
    if ((rc = dev_alloc(&c->d_conv, (size_t)mm * cc))) return rc;
    if ((rc = dev_alloc(&c->d_E, (size_t)mm))) return rc;
    if ((rc = dev_alloc(&c->d_w, (size_t)mm))) return rc;
    if ((rc = dev_alloc(&c->d_scal, (size_t)mm * 8))) return rc;
    c->m_cap = mm; c->contacts_cap = cc;
    return NEGF_OK;
}

SigmaProvider* get_provider(negf_ctx* c, int handle)
{
    if (!c || handle < 0 || handle >= (int)c->providers.size()) return nullptr;
    return c->providers[handle];
}

// A handle is the provider's index in a table that only grows: a freed slot stays empty and is never
// handed out again, so a stale handle (freed, or dropped by a change of the matrix dimension) can only
// ever name an empty slot -- negf_* calls then return NEGF_EINVAL instead of running on another
// object's self-energy.
int add_provider(negf_ctx* c, SigmaProvider* p)
{
    c->providers.push_back(p);
    return (int)c->providers.size() - 1;
}

// Python-style contact index normalisation; returns -1 for "total", -2 for invalid
int norm_contact(const SigmaProvider* p, int ind)
{
    if (ind == NEGF_IND_TOTAL) return -1;
    int nc = p->n_contacts;
    if (p->kind == SK_PRECOMPUTED) nc = std::max(p->pre_nc, 1);
    if (ind < 0) ind += nc;
    if (ind < 0 || ind >= nc) return -2;
    return ind;
}

// the terminals of a call with n_probes probes: the provider's contacts and the probes, TMAT_MAX_TERMINALS at most
bool probes_count_ok(const SigmaProvider* p, int n_probes)
{
    return n_probes >= 0 && (long)p->n_contacts + n_probes <= TMAT_MAX_TERMINALS;
}

int run_inverse(negf_ctx* c, int nb, int* info)
{
    ProfScope ps(c, "inverse");
    int algo = c->inverse_algo;
    c->G_deferred = false;
    c->gj_last = GjRecord{};
    c->gj_last.path = 0;                                         // (the unblocked kernel, unless the blocked launch says otherwise)
    if (algo == 0) algo = inverse_blocked_supported(c->n) ? 2 : 1;
    const int win_mode = algo == 3 ? 1 : algo == 4 ? 2 : 0;      // 3 / 4: the blocked path with the window kernel chosen
    if (algo > 2) algo = 2;
    bool in_b = false;
    if (algo == 2) {
        // false: no blocked kernel serves this n (nothing was launched) -> the unblocked kernel
        bool skip = c->defer_gather;
        in_b = launch_inverse_blocked(c->stream, c->n, nb, c->d_A, c->d_T1, (size_t)c->n * c->n, c->d_ipiv, info, &c->gj_side, win_mode, &skip, &c->gj_last);
        c->G_deferred = skip;
        if (!in_b) algo = 1;
    }
    if (algo == 1 && !launch_inverse_unblocked(c->stream, c->n, nb, c->d_A, info)) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipGetLastError());
    {   // 8 n^3 algorithmic; the blocked kernels run every rank-NB update on the matrix cores in 3M form over
        // 16-granular tiles with K in steps of four (the zero k-steps of a ragged last window are skipped); the pivot steps
        // themselves are vector work, and so is everything the strip window kernels do; the unblocked kernel issues none
        const double n = c->n, np = (double)((c->n + 15) & ~15), k4 = (double)((c->n + 3) & ~3);
        negf_count_flops(8.0 * n * n * n * nb, algo == 2 ? 6.0 * np * np * k4 * nb - inverse_blocked_vector_flops() : 0.0);
    }
    c->G = in_b ? c->d_T1 : c->d_A;
    c->W1 = in_b ? c->d_A : c->d_T1;
    c->W2 = c->d_T2;
    return NEGF_OK;
}

// One chain launch through the g(E) cache.  launch(g, mode) issues the solver's kernel: mode 2 on a hit -- only
// Sigma = t g t^H is formed from the entry's g, and the sweep counts and flags of the launch that filled the entry are
// copied out --, mode 1 otherwise, storing the final iterates into the entry when there is one to fill (g = nullptr: none).
template <typename Launch>
int chain_cached_launch(negf_ctx* c, ChainGEntry* ent, bool hit, int jobs, int* iters, int* conv, Launch launch)
{
    const size_t ib = (size_t)jobs * sizeof(int);
    if (hit) {
        launch(ent->d_g, 2);
        if (iters) NEGF_HIP_CHECK(hipMemcpyAsync(iters, ent->d_it, ib, hipMemcpyDeviceToDevice, c->stream));
        if (conv) NEGF_HIP_CHECK(hipMemcpyAsync(conv, ent->d_cv, ib, hipMemcpyDeviceToDevice, c->stream));
        return NEGF_OK;
    }
    if (ent && (!iters || !conv)) ent = nullptr;    // (an entry carries the counts and flags of its launch)
    launch(ent ? ent->d_g : nullptr, 1);
    if (ent) {
        NEGF_HIP_CHECK(hipMemcpyAsync(ent->d_it, iters, ib, hipMemcpyDeviceToDevice, c->stream));
        NEGF_HIP_CHECK(hipMemcpyAsync(ent->d_cv, conv, ib, hipMemcpyDeviceToDevice, c->stream));
        NEGF_HIP_CHECK(hipGetLastError());                 // an entry whose launch failed never becomes a hit
        ent->valid = true;
    }
    return NEGF_OK;
}

// The job order of a fixed-point chain launch, learned from the provider's previous evaluation.
// Jobs run in the order of decreasing sweep counts: the counts are predicted from the previous evaluation of this
// provider -- for each energy the count of the nearest energy evaluated then (Fermi searches and SCF cycles evaluate
// the same or slightly moved grids over and over; the same grid gets exactly its learned order) -- and sorted on the
// device, no host sync; the first evaluation runs in launch order.  What the order is for: a launch with FEWER jobs
// than resident slots (the SCF-sized grids) is dispatched to the compute units in this order, so the long jobs are
// spread over the chip instead of sharing a unit with their neighbours in energy (648 jobs: 42 against 48 ms); a
// launch with MORE jobs runs them round robin (k_chain1d_rs.hip), where the initial content of the queue is worth
// nothing (C3 grid: 576.4 ms per step in the learned order, 576.1 ms in launch order), so no order is predicted for it.
// record = false, before the launch: *order = the predicted order (nullptr: launch order); order = nullptr: the launch
// takes no order, only the record of the previous evaluation is promoted.
// record = true, after it: the chunk's energies and counts are appended to the record of the evaluation in progress.
int chain_learn_order(negf_ctx* c, SigmaProvider* p, int nb, const cplx* E, const int* iters, int m0, bool record,
                      const int** order = nullptr)
{
    const int jobs = nb * p->n_contacts;
    if (!record) {
        if (m0 == 0 && p->cur_n > 0) {
            // a new evaluation begins: the one recorded so far becomes the reference
            std::swap(p->d_prevE, p->d_curE); std::swap(p->d_prev_iters, p->d_cur_iters);
            std::swap(p->prev_cap, p->cur_cap);
            p->prev_n = p->cur_n; p->cur_n = 0;
        }
        if (!order) return NEGF_OK;
        int rc = ensure_cap(c, p->d_order, (size_t)jobs);
        if (rc) return rc;
        if (p->prev_n > 0) {
            launch_chain1d_predict_order(c->stream, p->d_prevE, p->d_prev_iters, p->prev_n, p->n_contacts, E, nb, p->d_order);
            *order = p->d_order;
        } else if (p->cur_n > 0) {
            // the first evaluation ever, arriving in chunks: the chunks so far are all there is to learn from
            launch_chain1d_predict_order(c->stream, p->d_curE, p->d_cur_iters, p->cur_n, p->n_contacts, E, nb, p->d_order);
            *order = p->d_order;
        }
        return NEGF_OK;
    }
    if (m0 != 0 && m0 != p->cur_n) return NEGF_OK;
    if (m0 == 0) p->cur_n = 0;
    if (m0 + nb > p->cur_cap) {
        const int cap = std::max(m0 + nb, 2 * p->cur_cap);
        cplx* nE = nullptr; int* nI = nullptr;
        int rc;
        if ((rc = dev_alloc(&nE, (size_t)cap)) || (rc = dev_alloc(&nI, (size_t)cap * p->n_contacts))) { dev_free(nE); return rc; }
        if (p->cur_n > 0) {
            NEGF_HIP_CHECK(hipMemcpyAsync(nE, p->d_curE, (size_t)p->cur_n * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream));
            NEGF_HIP_CHECK(hipMemcpyAsync(nI, p->d_cur_iters, (size_t)p->cur_n * p->n_contacts * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        }
        NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
        dev_free(p->d_curE); dev_free(p->d_cur_iters);
        p->d_curE = nE; p->d_cur_iters = nI; p->cur_cap = cap;
    }
    NEGF_HIP_CHECK(hipMemcpyAsync(p->d_curE + m0, E, (size_t)nb * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream));
    NEGF_HIP_CHECK(hipMemcpyAsync(p->d_cur_iters + (size_t)m0 * p->n_contacts, iters, (size_t)jobs * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    p->cur_n = m0 + nb;
    return NEGF_OK;
}

// Sigma blocks of a block provider for energies E[0..nb) -> c->d_blk
// (m0 = position of this chunk in the grid being evaluated: the sweep-count prediction keeps whole evaluations)
// blk_out: another destination [nb][blk_stride] (the terminals of a layered system keep their own)
int run_sigma_blocks(negf_ctx* c, SigmaProvider* p, int nb, const cplx* E, int* iters, int* conv, int m0, cplx* blk_out = nullptr)
{
    cplx* const blk = blk_out ? blk_out : c->d_blk.p;
    if (p->kind == SK_BETHE) {
        ProfScope ps(c, "bethe");
        launch_bethe(c->stream, *p, nb, E, blk, iters, conv);
        return NEGF_OK;
    }
    if (p->kind != SK_CHAIN1D) return NEGF_OK;
    static int force_v1 = -1;
    if (force_v1 < 0) { const char* e = getenv("NEGF_CHAIN1D_ALGO"); force_v1 = (e && strcmp(e, "global") == 0) ? 1 : 0; }
    const bool rd = p->solver == 1;       // renormalisation-decimation: one launch, no job order (units differ by at most a factor two in length)
    const bool lds_path = chain1d_lds_supported(p->nc_max) && (!force_v1 || rd);
    // the g(E) cache (ChainGEntry): a launch whose lead and energies were evaluated before only forms Sigma = t g t^H
    ChainGEntry* ent = nullptr;
    bool hit = false;
    struct Pin { negf_ctx* c; ~Pin() { c->gcache_pinned = false; } } pin{c};      // `ent` points into the cache until this function ends
    c->gcache_pinned = true;
    if (lds_path && c->gcache_max > 0) {
        std::vector<cplx> tmp;
        ent = gcache_lookup(c, p, host_energies(c, E, nb, tmp), nb, &hit);
    }
    ProfScope ps(c, rd ? (hit ? "chain1d_rd_hit" : "chain1d_rd") : (hit ? "chain1d_hit" : "chain1d"));
    const size_t per = rd || lds_path ? 0 : chain1d_scratch_per_wg(p->nc_max);
    int rc = ensure_cap(c, c->d_scratch,
                        rd ? chain1d_rd_scratch_elems(p->nc_max, p->n_contacts, nb)
                        : lds_path ? chain1d_lds_scratch_elems(p->nc_max, p->n_contacts, nb, std::max(p->max_iter, p->force_iters), c->chain_rr_quantum)
                                   : per * p->n_contacts * nb);
    if (rc) return rc;
    const int jobs = nb * p->n_contacts;
    if (rd)
        return chain_cached_launch(c, ent, hit, jobs, iters, conv, [&](cplx* g, int mode) {
            launch_chain1d_rd(c->stream, *p, p->d_nc, p->d_blk_off, nb, E, blk, iters, conv, c->d_scratch, g, mode);
        });
    if (!lds_path) {
        launch_chain1d(c->stream, *p, p->d_nc, p->d_blk_off, nb, E, blk, iters, conv, c->d_scratch, per);
        return NEGF_OK;
    }
    const bool learn = !hit && p->force_iters < 0 && iters && chain1d_order_supported(jobs);
    // (a launch with more jobs than resident slots runs round robin and takes no order)
    const int* order = nullptr;
    const bool queue = chain1d_lds_runs_queue(*p, nb, c->chain_rr_quantum, c->chain_rr_slots);
    if (learn && (rc = chain_learn_order(c, p, nb, E, iters, m0, false, queue ? nullptr : &order))) return rc;
    rc = chain_cached_launch(c, ent, hit, jobs, iters, conv, [&](cplx* g, int mode) {
        if (mode == 2) launch_chain1d_lds(c->stream, *p, p->d_nc, p->d_blk_off, nb, E, blk, iters, conv, c->d_scratch, nullptr, g, 2);
        else launch_chain1d_lds(c->stream, *p, p->d_nc, p->d_blk_off, nb, E, blk, iters, conv, c->d_scratch, order, g, 1,
                                c->chain_rr_quantum, c->chain_rr_slots);
    });
    if (rc || !learn) return rc;
    return chain_learn_order(c, p, nb, E, iters, m0, true);
}

// assemble A_b = E_b S - F - Sigma_b for batch [m0, m0+nb) into c->d_A
int run_assemble(negf_ctx* c, SigmaProvider* p, int m0, int nb, const cplx* E)
{
    int rc = NEGF_OK;
    if (p->kind == SK_CHAIN1D || p->kind == SK_BETHE) {
        rc = run_sigma_blocks(c, p, nb, E + m0, c->d_iters + (size_t)m0 * p->n_contacts,
                              c->d_conv + (size_t)m0 * p->n_contacts, m0);
        if (rc) return rc;
    }
    ProfScope ps(c, "assemble");
    const size_t n2 = (size_t)c->n * c->n;
    switch (p->kind) {
    case SK_CONST:
        launch_assemble(c->stream, c->n, nb, E + m0, c->d_S, p->d_hbase, nullptr, nullptr, 0, 0,
                        nullptr, nullptr, nullptr, nullptr, c->d_A);
        break;
    case SK_PRECOMPUTED:
        launch_assemble(c->stream, c->n, nb, E + m0, c->d_S, c->d_F, p->d_pre_tot + n2 * m0, nullptr, 0,
                        0, nullptr, nullptr, nullptr, nullptr, c->d_A);
        break;
    case SK_CHAIN1D:
    case SK_BETHE:
        if (p->d_xi) {
            // Sigma = Xi blockdiag Xi (surfGBethe.py:530-533): dense via two products
            launch_scatter_blocks(c->stream, c->n, nb, c->d_blk, p->blk_stride, p->n_contacts, p->d_nc,
                                  p->d_blk_off, p->d_inds_off, p->d_inds, -1, c->d_T1);
            launch_zgemm(c->stream, c->n, c->n, c->n, nb, p->d_xi, c->n, 0, c->d_T1, c->n, n2, 0,
                         c->d_T2, c->n, n2);
            launch_zgemm(c->stream, c->n, c->n, c->n, nb, c->d_T2, c->n, n2, p->d_xi, c->n, 0, 0,
                         c->d_T1, c->n, n2);
            launch_assemble(c->stream, c->n, nb, E + m0, c->d_S, c->d_F, c->d_T1, nullptr, 0, 0, nullptr,
                            nullptr, nullptr, nullptr, c->d_A);
        } else {
            launch_assemble(c->stream, c->n, nb, E + m0, c->d_S, c->d_F, nullptr, c->d_blk, p->blk_stride,
                            p->n_contacts, p->d_nc, p->d_blk_off, p->d_inds_off, p->d_inds, c->d_A);
        }
        break;
    default:
        return NEGF_EINVAL;
    }
    return NEGF_OK;
}

// G(E) for the batch [m0, m0 + nb): assemble + inverse, leaving c->G / c->W1 / c->W2 set.  Small systems take the
// fused kernel in STORE mode (one launch, the matrix stays on the CU; k_small_fused.hip).
int run_assemble_inverse(negf_ctx* c, SigmaProvider* p, int m0, int nb, const cplx* E)
{
    int rc;
    if (small_path(c, p)) {
        if (p->kind == SK_CHAIN1D || p->kind == SK_BETHE) {
            if ((rc = run_sigma_blocks(c, p, nb, E + m0, c->d_iters + (size_t)m0 * p->n_contacts,
                                       c->d_conv + (size_t)m0 * p->n_contacts, m0))) return rc;
        }
        ProfScope ps(c, "small");
        SmallFusedArgs a = small_args(c, p, m0, nb, E);
        a.Gout = c->d_A; a.g_stride = (size_t)c->n * c->n;
        launch_small_fused(c->stream, a);
        negf_count_flops(8.0 * c->n * (double)c->n * c->n * nb, 0.0);
        NEGF_HIP_CHECK(hipGetLastError());
        c->G = c->d_A; c->W1 = c->d_T1; c->W2 = c->d_T2;
        return NEGF_OK;
    }
    if ((rc = run_assemble(c, p, m0, nb, E))) return rc;
    return run_inverse(c, nb, c->d_info + m0);
}

// dense Gamma_b = i (Sigma_c - Sigma_c^H) for batch [m0, m0+nb) into `out`
// (stride n*n); returns the batch stride to use (0 when one matrix serves all).
int run_gamma(negf_ctx* c, SigmaProvider* p, int contact /* -1 total */, int m0, int nb, cplx* out,
              cplx* scratch, const cplx** gptr, size_t* stride_out)
{
    const size_t n2 = (size_t)c->n * c->n;
    *gptr = out;
    if (p->kind == SK_PRECOMPUTED && p->pre_is_gamma) {
        // the caller supplied the coupling matrices themselves (transport.py:150-181 take
        // gamma1/gamma2 as arguments): use them in place
        if (contact < 0 || !p->d_pre_c) return NEGF_EINVAL;
        *gptr = p->d_pre_c + n2 * ((size_t)m0 * p->pre_nc + contact);
        *stride_out = n2 * p->pre_nc;
        return NEGF_OK;
    }
    switch (p->kind) {
    case SK_CONST: {
        const cplx* src = contact < 0 ? p->d_const_tot : p->d_const_c + n2 * contact;
        launch_gamma_dense(c->stream, c->n, 1, src, 0, out);
        *stride_out = 0;
        return NEGF_OK;
    }
    case SK_PRECOMPUTED: {
        if (contact < 0 || !p->d_pre_c) {
            launch_gamma_dense(c->stream, c->n, nb, p->d_pre_tot + n2 * m0, n2, out);
        } else {
            const int pn = std::max(p->pre_nc, 1);
            launch_gamma_dense(c->stream, c->n, nb, p->d_pre_c + n2 * ((size_t)m0 * pn + contact),
                               n2 * pn, out);
        }
        *stride_out = n2;
        return NEGF_OK;
    }
    case SK_CHAIN1D:
    case SK_BETHE: {
        // c->d_blk holds the blocks of this batch (run_assemble was just called)
        launch_scatter_blocks(c->stream, c->n, nb, c->d_blk, p->blk_stride, p->n_contacts, p->d_nc,
                              p->d_blk_off, p->d_inds_off, p->d_inds, contact, out);
        if (p->d_xi) {
            // Xi sig Xi through the scratch area
            launch_zgemm(c->stream, c->n, c->n, c->n, nb, p->d_xi, c->n, 0, out, c->n, n2, 0, scratch,
                         c->n, n2);
            launch_zgemm(c->stream, c->n, c->n, c->n, nb, scratch, c->n, n2, p->d_xi, c->n, 0, 0, out,
                         c->n, n2);
        }
        // the gamma kernel reads s[t] and s[transpose]: not in place -> via scratch
        launch_gamma_dense(c->stream, c->n, nb, out, n2, scratch);
        (void)hipMemcpyAsync(out, scratch, n2 * nb * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream);
        *stride_out = n2;
        return NEGF_OK;
    }
    }
    return NEGF_EINVAL;
}

// ---- compact coupling matrices (see k_elementwise.hip): usable when Gamma_c is confined to the
// contact's index list and all lists together cover at most half of the orbitals
bool compact_available(const negf_ctx* c, const SigmaProvider* p)
{
    if (c->gamma_algo == 1) return false;
    if (p->kind == SK_CONST) return p->compact_ok;
    if ((p->kind == SK_CHAIN1D || p->kind == SK_BETHE) && !p->d_xi) {
        int tot = 0;
        for (int k : p->nc) tot += k;
        return 2 * tot <= c->n;
    }
    return false;
}

struct GammaSmall { const cplx* mat; size_t stride; const int* idx; int K; };

// small Gamma of `contact` (or of all contacts, block diagonal, for contact < 0) for the batch
// [m0, m0+nb) into slot `slot` (0/1) of c->d_gsmall
int run_gamma_small(negf_ctx* c, SigmaProvider* p, int contact, int nb, int slot, GammaSmall* g)
{
    const int c0 = contact < 0 ? 0 : contact, c1 = contact < 0 ? p->n_contacts : contact + 1;
    int K = 0;
    for (int k = c0; k < c1; ++k) K += p->nc[k];
    int Kmax = 0;
    for (int k : p->nc) Kmax += k;
    if (int rc = ensure_cap(c, c->d_gsmall, (size_t)2 * nb * Kmax * Kmax)) return rc;
    cplx* out = c->d_gsmall + (size_t)slot * nb * Kmax * Kmax;
    const bool constant = p->kind == SK_CONST;
    launch_gamma_small(c->stream, K, c0, c1, constant ? 1 : nb, p->d_nc, p->d_blk_off, p->d_inds_off,
                       constant ? p->d_const_blk : c->d_blk.p, constant ? 0 : (size_t)p->blk_stride, out,
                       (size_t)K * K);
    g->mat = out; g->stride = constant ? 0 : (size_t)K * K; g->idx = p->d_inds + p->inds_off[c0]; g->K = K;
    return NEGF_OK;
}

int check_ready(negf_ctx* c, SigmaProvider* p, int m)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (!p) return NEGF_EINVAL;
    if (m < 0) return NEGF_EINVAL;
    if (p->kind == SK_PRECOMPUTED && m > p->m_pre) return NEGF_EINVAL;
    return NEGF_OK;
}

// What opens an entry point that evaluates a provider: the handle is resolved, check_ready decides between NEGF_ESTATE
// and NEGF_EINVAL, the contact indices the entry point names (indA -> *ctA, indB -> *ctB; nullptr: none) are normalised
// and invalid ones refused, and the context's device is selected.  The entry point's own argument checks follow.
int open_call(negf_ctx* c, int handle, int m, SigmaProvider** p, int indA = 0, int* ctA = nullptr, int indB = 0, int* ctB = nullptr)
{
    *p = get_provider(c, handle);
    int rc = check_ready(c, *p, m);
    if (rc) return rc;
    if (ctA && (*ctA = norm_contact(*p, indA)) == -2) return NEGF_EINVAL;
    if (ctB && (*ctB = norm_contact(*p, indB)) == -2) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    return NEGF_OK;
}

// sweep counts and flags [m][n_contacts] of the last evaluation of p (either may be null); a provider without a fixed
// point: none run, all converged
int fetch_iters(negf_ctx* c, const SigmaProvider* p, int m, int* iters, int* converged)
{
    const size_t cnt = (size_t)m * p->n_contacts;
    int rc;
    if (p->kind == SK_CHAIN1D || p->kind == SK_BETHE) {
        if (iters && (rc = download(c, iters, c->d_iters, cnt))) return rc;
        if (converged && (rc = download(c, converged, c->d_conv, cnt))) return rc;
        return NEGF_OK;
    }
    for (size_t i = 0; i < cnt; ++i) { if (iters) iters[i] = 0; if (converged) converged[i] = 1; }
    return NEGF_OK;
}

// assemble + inverse for a weighted sum of G, which needs no G itself: the windowed inverse leaves its gather out and
// the sum reads the reduced matrices through the pivot bookkeeping.  *perm: that is how the result was left (in c->W1,
// with c->d_ipiv); otherwise it is in c->G as usual.
int run_inverse_for_sum(negf_ctx* c, SigmaProvider* p, int m0, int nb, const cplx* E, bool* perm)
{
    c->defer_gather = true;
    const int rc = run_assemble_inverse(c, p, m0, nb, E);
    c->defer_gather = false;
    *perm = c->G_deferred;
    c->G_deferred = false;
    return rc;
}

// the share of every segment (consecutive, ending at seg_end[s]) in the batch [m0, m0 + nb): energies [lo, hi) of the
// batch, counted from its first one, belong to segment slot; empty shares are left out
struct SegShares { std::vector<int> lo, hi, slot; };
SegShares batch_shares(int nseg, const int* seg_end, int m0, int nb)
{
    SegShares sh;
    for (int sg = 0, start = 0; sg < nseg; start = seg_end[sg], ++sg) {
        const int lo = std::max(start, m0), hi = std::min(seg_end[sg], m0 + nb);
        if (hi > lo) { sh.lo.push_back(lo - m0); sh.hi.push_back(hi - m0); sh.slot.push_back(sg); }
    }
    return sh;
}

int reduce_info(negf_ctx* c, int m, int* info_host)
{
    if (m == 0) return NEGF_OK;
    std::vector<int> tmp;
    int* dst = info_host;
    if (!dst) { tmp.resize(m); dst = tmp.data(); }
    int rc = download(c, dst, c->d_info, (size_t)m);
    if (rc) return rc;
    for (int i = 0; i < m; ++i) if (dst[i] != 0) return NEGF_ESINGULAR;
    return NEGF_OK;
}

// how a device-resident call ends once everything is queued: the grid length noted, a launch error reported
int close_call(negf_ctx* c, int m)
{
    c->last_m = m;
    NEGF_HIP_CHECK(hipGetLastError());
    return NEGF_OK;
}

// The batches of a call that sweeps the n x n workspace over a grid of m energies, the dense twin of rgf_batches
// (negf_layered_impl.h): the per-energy buffers and the workspace stand (ensure_workspace may set c->batch: it is read
// after it), setup(batch) runs once -- what the call sizes by the batch or queues in front of its first batch --, then
// body(m0, nb) per batch [m0, m0 + nb); the first nonzero rc ends the call.  An entry point that treats m == 0 on its
// own (an early return, a result to clear) does so before it gets here.  Not its clients:
//   - the small_path branches of negf_gr_int_dev and gr_seg_core: one fused kernel per chunk of SMALL_CHUNK energies
//     (per call for the segments) and no n x n workspace;
//   - negf_transmission_dev: a workspace of two energies at least, swept by HALF the batch (the other half is scratch).
template <class Setup, class Body>
int dense_batches(negf_ctx* c, SigmaProvider* p, int m, Setup&& setup, Body&& body)
{
    int rc;
    if ((rc = ensure_mbuffers(c, m, p->n_contacts)) || (rc = ensure_workspace(c, m, p->blk_stride))) return rc;
    const int batch = c->batch;
    if ((rc = setup(batch))) return rc;
    for (int m0 = 0; m0 < m; m0 += batch)
        if ((rc = body(m0, std::min(batch, m - m0)))) return rc;
    return close_call(c, m);
}
template <class Body>
int dense_batches(negf_ctx* c, SigmaProvider* p, int m, Body&& body)
{
    return dense_batches(c, p, m, [](int) { return NEGF_OK; }, body);
}

// the setup of a call that sums into `out`: cleared in front of the first batch
auto clear_first(negf_ctx* c, void* out, size_t bytes)
{
    return [=](int) -> int { NEGF_HIP_CHECK(hipMemsetAsync(out, 0, bytes, c->stream)); return NEGF_OK; };
}

}  // namespace

void free_layered(LayeredSystem* ls);      // negf_layered_impl.h

// =========================================================================== //
extern "C" {

int negf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

const char* negf_version(void) { return "gaunegf_amd-0.1 (gfx950)"; }

const char* negf_strerror(int code)
{
    switch (code) {
    case NEGF_OK: return "ok";
    case NEGF_EINVAL: return "invalid argument";
    case NEGF_ENOMEM: return "out of device memory";
    case NEGF_EHIP: return "HIP runtime error";
    case NEGF_ENODEV: return "no HIP device available (this library has no CPU fallback)";
    case NEGF_ESTATE: return "call negf_set_system first";
    case NEGF_ESINGULAR: return "exactly singular matrix at one or more energies (see info[])";
    default: return "unknown error";
    }
}

int negf_create(negf_ctx** out, int device)
{
    if (!out) return NEGF_EINVAL;
    *out = nullptr;
    const int nd = negf_device_count();
    if (nd <= 0) return NEGF_ENODEV;
    if (device < 0 || device >= nd) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(device));
    negf_ctx* c = new (std::nothrow) negf_ctx();
    if (!c) return NEGF_ENOMEM;
    c->device = device;
    if (const char* e = getenv("NEGF_CHAIN_CACHE")) c->gcache_max = std::min(std::max(atoi(e), 0), 4096);   // default of negf_set_chain_cache
    c->gcache.reserve((size_t)c->gcache_max);
    live_contexts().push_back(c);
    *out = c;
    return NEGF_OK;
}

void negf_destroy(negf_ctx* c)
{
    if (!c) return;
    { auto& v = live_contexts(); v.erase(std::remove(v.begin(), v.end(), c), v.end()); }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto* p : c->providers) free_provider(p);
    for (auto* ls : c->layered) free_layered(ls);
    free_workspace(c, true); free_mbuffers(c); free_gcache(c);
    free_pinned(c);
    for (auto& sl : c->sys) { dev_free(sl.dF); dev_free(sl.dS); }
    c->d_F = c->d_S = nullptr;
    dev_free(c->d_acc); dev_free(c->d_ref_meta);
    prof_resolve(c);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    delete c;
}

int negf_set_stream(negf_ctx* c, void* s)
{
    if (!c) return NEGF_EINVAL;
    hipStream_t next = reinterpret_cast<hipStream_t>(s);
    if (next == c->stream) return NEGF_OK;                 // (bench.py's workers call this once each: no runtime call)
    // Work queued on the old stream still owns the context's work areas (d_A, d_T1, d_T2, d_ipiv, d_info, d_acc, the
    // pinned staging buffer, the g(E) cache entries), and every host-side decision of this file (ensure_cap, ensure_pinned,
    // the cache eviction, negf_destroy) waits for c->stream alone: the new stream is ordered BEHIND the old one with an
    // event, on the device, so that c->stream stays the one stream whose completion covers everything in flight.  The
    // host does not wait.  (The wait takes the event's state at this call: the event goes back to the pool at once.)
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    hipEvent_t e = prof_get_event(c);
    if (!e) return NEGF_EHIP;
    hipError_t err = hipEventRecord(e, c->stream);
    if (err == hipSuccess) err = hipStreamWaitEvent(next, e, 0);
    c->ev_pool.push_back(e);
    NEGF_HIP_CHECK(err);
    c->stream = next;
    return NEGF_OK;
}

int negf_set_batch(negf_ctx* c, int batch)
{
    if (!c || batch < 0) return NEGF_EINVAL;
    c->batch_user = batch;
    return NEGF_OK;
}
int negf_get_batch(negf_ctx* c) { return c ? c->batch : 0; }

int negf_set_inverse_algo(negf_ctx* c, int algo)
{
    if (!c || algo < 0 || algo > 4) return NEGF_EINVAL;
    c->inverse_algo = algo;
    return NEGF_OK;
}

int negf_set_small_algo(negf_ctx* c, int algo)
{
    if (!c || algo < 0 || algo > 1) return NEGF_EINVAL;
    c->small_algo = algo;
    return NEGF_OK;
}

int negf_set_chain_round_robin(negf_ctx* c, int quantum, int slots)
{
    if (!c || slots < 0) return NEGF_EINVAL;
    c->chain_rr_quantum = quantum < 0 ? -1 : quantum;
    c->chain_rr_slots = slots;
    return NEGF_OK;
}

int negf_set_gamma_algo(negf_ctx* c, int algo)
{
    if (!c || algo < 0 || algo > 1) return NEGF_EINVAL;
    c->gamma_algo = algo;
    return NEGF_OK;
}

// bitwise comparison of two host buffers; large ones in parallel chunks (a 2 x 10 MB comparison per integral is 2 ms of the
// 11 ms a per-GPU share of BASELINE C4 leaves an entry point; a different system differs within the first bytes: the
// first chunk is compared alone before the threads are started)
static bool same_bytes(const void* a, const void* b, size_t bytes)
{
    const size_t head = std::min<size_t>(bytes, (size_t)1 << 16);
    if (std::memcmp(a, b, head) != 0) return false;
    if (bytes <= ((size_t)1 << 21)) return std::memcmp(a, b, bytes) == 0;
    const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const size_t chunk = (bytes + hw - 1) / hw;
    std::atomic<bool> same{true};
    std::vector<std::thread> th;
    try {
        for (unsigned t = 1; t < hw; ++t) {
            const size_t lo = std::min(bytes, t * chunk), hi = std::min(bytes, lo + chunk);
            if (hi <= lo) break;
            th.emplace_back([&same, a, b, lo, hi] { if (std::memcmp((const char*)a + lo, (const char*)b + lo, hi - lo) != 0) same = false; });
        }
    } catch (...) {                                              // (no more threads: the rest is compared here)
    }
    const size_t mine_hi = std::min(bytes, chunk);
    if (std::memcmp(a, b, mine_hi) != 0) same = false;
    if (th.size() + 1 < hw) {                                    // chunks nobody took
        const size_t lo = std::min(bytes, (th.size() + 1) * chunk);
        if (lo < bytes && std::memcmp((const char*)a + lo, (const char*)b + lo, bytes - lo) != 0) same = false;
    }
    for (auto& x : th) x.join();
    return same;
}

// host copy of a result out of the pinned staging buffer; results of several MB (an 800 x 800 matrix is 10 MB: 1.3 ms of a
// 14-ms entry point on one core) in parallel chunks
static void copy_bytes(void* dst, const void* src, size_t bytes)
{
    if (bytes < ((size_t)1 << 22)) { std::memcpy(dst, src, bytes); return; }
    constexpr unsigned NT = 8;
    const size_t chunk = (((bytes + NT - 1) / NT) + 63) / 64 * 64;
    std::vector<std::thread> th;
    size_t done_to = std::min(bytes, chunk);                     // [0, chunk) is this thread's
    try {
        for (unsigned t = 1; t < NT; ++t) {
            const size_t lo = std::min(bytes, t * chunk), hi = std::min(bytes, lo + chunk);
            if (hi <= lo) break;
            th.emplace_back([dst, src, lo, hi] { std::memcpy((char*)dst + lo, (const char*)src + lo, hi - lo); });
            done_to = hi;
        }
    } catch (...) {                                              // (no more threads: the rest is copied here)
    }
    std::memcpy(dst, src, std::min(bytes, chunk));
    if (done_to < bytes) std::memcpy((char*)dst + done_to, (const char*)src + done_to, bytes - done_to);
    for (auto& x : th) x.join();
}

// 64-bit checksum of a host buffer (change detection for the front end's caches, not cryptography): four independent
// multiply-xorshift lanes per chunk, large buffers in parallel chunks, the chunk values folded in order
static unsigned long long hash_chunk(const unsigned char* p, size_t bytes)
{
    const unsigned long long K = 0x9E3779B97F4A7C15ull;
    unsigned long long h[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32) {
        unsigned long long x[4];
        std::memcpy(x, p + i, 32);
        for (int l = 0; l < 4; ++l) { h[l] = (h[l] ^ x[l]) * K; h[l] ^= h[l] >> 32; }
    }
    unsigned long long tail[4] = {0, 0, 0, 0};
    if (i < bytes) {
        std::memcpy(tail, p + i, bytes - i);
        for (int l = 0; l < 4; ++l) { h[l] = (h[l] ^ tail[l]) * K; h[l] ^= h[l] >> 32; }
    }
    unsigned long long r = bytes * K;
    for (int l = 0; l < 4; ++l) { r = (r ^ h[l]) * K; r ^= r >> 29; }
    return r;
}

unsigned long long negf_hash_bytes(const void* data, unsigned long long bytes)
{
    if (!data || bytes == 0) return 0x9E3779B97F4A7C15ull;
    const unsigned char* p = static_cast<const unsigned char*>(data);
    if (bytes < ((size_t)1 << 21)) return hash_chunk(p, (size_t)bytes);
    constexpr unsigned NT = 8;
    const size_t chunk = ((((size_t)bytes + NT - 1) / NT) + 31) / 32 * 32;
    unsigned long long part[NT] = {0};
    std::vector<std::thread> th;
    unsigned started = 1;
    try {
        for (unsigned t = 1; t < NT; ++t) {
            const size_t lo = std::min<size_t>(bytes, t * chunk), hi = std::min<size_t>(bytes, lo + chunk);
            if (hi <= lo) break;
            th.emplace_back([&part, p, lo, hi, t] { part[t] = hash_chunk(p + lo, hi - lo); });
            started = t + 1;
        }
    } catch (...) {                                              // (no more threads: the rest is hashed here)
    }
    part[0] = hash_chunk(p, std::min<size_t>(bytes, chunk));
    for (unsigned t = started; t < NT; ++t) {                    // chunks nobody took
        const size_t lo = std::min<size_t>(bytes, t * chunk), hi = std::min<size_t>(bytes, lo + chunk);
        if (hi > lo) part[t] = hash_chunk(p + lo, hi - lo);
    }
    for (auto& x : th) x.join();
    return hash_chunk(reinterpret_cast<const unsigned char*>(part), sizeof(part)) ^ bytes;
}

int negf_set_system(negf_ctx* c, int n, const double* F, const double* S)
{
    return negf_set_system_keyed(c, n, F, S, 0ull);
}

int negf_set_system_keyed(negf_ctx* c, int n, const double* F, const double* S, unsigned long long key)
{
    if (!c || n <= 0 || !F || !S) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t n2 = (size_t)n * n;
    int rc;
    if (n != c->n) {
        // providers are tied to the matrix dimension
        for (auto*& p : c->providers) { free_provider(p); p = nullptr; }
        free_workspace(c);
        for (auto& sl : c->sys) { dev_free(sl.dF); dev_free(sl.dS); sl.valid = false; sl.hF.clear(); sl.hS.clear(); }
        c->d_F = c->d_S = nullptr; c->sys_cur = -1;
        dev_free(c->d_acc);
        c->n = n;
        if ((rc = dev_alloc(&c->d_acc, n2))) return rc;
    }
    const cplx* Fh = reinterpret_cast<const cplx*>(F);
    const cplx* Sh = reinterpret_cast<const cplx*>(S);
    // one of the systems already on the device?  (bitwise comparison with the host copies; matrices above 256 MB
    // -- n > 4096 -- keep one system only: a slot costs 2 x 16 n^2 bytes of HBM and of host memory)
    const int nslots = n2 * sizeof(cplx) <= ((size_t)256 << 20) ? negf_ctx::NEGF_SYS_SLOTS : 1;
    int slot = -1;
    // (a caller's key: equal keys vouch for bitwise-equal contents -- the front end's private, immutable copies -- and
    //  select a resident system without the 2 x 16 n^2 bytes of comparison)
    if (key)
        for (int k = 0; k < nslots && slot < 0; ++k)
            if (c->sys[k].valid && c->sys[k].hF.size() == n2 && c->sys[k].key == key) slot = k;
    for (int k = 0; k < nslots && slot < 0; ++k) {
        auto& sl = c->sys[k];
        if (sl.valid && sl.hF.size() == n2 && same_bytes(sl.hF.data(), Fh, n2 * sizeof(cplx)) &&
            same_bytes(sl.hS.data(), Sh, n2 * sizeof(cplx))) { slot = k; sl.key = key; }
    }
    if (slot >= 0 && slot == c->sys_cur) return NEGF_OK;             // resident: nothing to do
    if (slot < 0) {
        // least recently used slot (an empty one first)
        slot = 0;
        for (int k = 1; k < nslots; ++k)
            if (!c->sys[k].valid ? c->sys[slot].valid : (c->sys[slot].valid && c->sys[k].used < c->sys[slot].used)) slot = k;
        auto& sl = c->sys[slot];
        sl.valid = false;
        if (!sl.dF && (rc = dev_alloc(&sl.dF, n2))) return rc;
        if (!sl.dS && (rc = dev_alloc(&sl.dS, n2))) return rc;
        if ((rc = upload(c, sl.dF, Fh, n2))) return rc;
        if ((rc = upload(c, sl.dS, Sh, n2))) return rc;
        sl.hF.assign(Fh, Fh + n2);
        sl.hS.assign(Sh, Sh + n2);
        sl.key = key;
        sl.valid = true;
    }
    c->sys[slot].used = ++c->sys_clock;
    c->sys_cur = slot;
    c->d_F = c->sys[slot].dF;
    c->d_S = c->sys[slot].dS;
    // constant providers cache F + Sigma_tot: refresh them for the resident F (on the device, same rounding as
    // the host sum at creation: one IEEE addition per component)
    for (auto* p : c->providers)
        if (p && p->kind == SK_CONST) launch_cadd(c->stream, n2, c->d_F, p->d_const_tot, p->d_hbase);
    NEGF_HIP_CHECK(hipGetLastError());
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return NEGF_OK;
}

// ------------------------------------------------------------------ providers
static int setup_blocks(negf_ctx* c, SigmaProvider* p, int n_contacts, const int* nc, const int* inds, int n = -1);

int negf_sigma_const(negf_ctx* c, int n_contacts, const double* sigma, int* handle)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (n_contacts <= 0 || !sigma || !handle) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    const size_t n2 = (size_t)c->n * c->n;
    SigmaProvider* p = new SigmaProvider();
    p->kind = SK_CONST; p->n_contacts = n_contacts;
    int rc;
    if ((rc = dev_alloc(&p->d_const_c, n2 * n_contacts)) || (rc = dev_alloc(&p->d_const_tot, n2)) ||
        (rc = dev_alloc(&p->d_hbase, n2))) { free_provider(p); return rc; }
    const cplx* s = reinterpret_cast<const cplx*>(sigma);
    // total = sum over contacts in contact order (surfGTester.py:128-131); F + total
    // is a host-side O(n^2) setup step, the per-energy work stays on the GPU
    std::vector<cplx> tot(n2, cmake(0.0, 0.0)), hb(n2), Fh(n2);
    for (int k = 0; k < n_contacts; ++k)
        for (size_t i = 0; i < n2; ++i) tot[i] = cadd(tot[i], s[k * n2 + i]);
    if ((rc = download(c, Fh.data(), c->d_F, n2))) { free_provider(p); return rc; }
    for (size_t i = 0; i < n2; ++i) hb[i] = cadd(Fh[i], tot[i]);
    if ((rc = upload(c, p->d_const_c, s, n2 * n_contacts)) || (rc = upload(c, p->d_const_tot, tot.data(), n2)) ||
        (rc = upload(c, p->d_hbase, hb.data(), n2))) { free_provider(p); return rc; }
    // support of each contact matrix (rows or columns holding a nonzero): formSigma-style contacts
    // (matTools.py:90-120) only touch their own orbitals, so Gamma_c is a small block
    {
        const int n = c->n;
        std::vector<int> ks(n_contacts), inds;
        for (int k = 0; k < n_contacts; ++k) {
            const cplx* m = s + (size_t)k * n2;
            std::vector<char> used(n, 0);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    if (m[(size_t)i * n + j].x != 0.0 || m[(size_t)i * n + j].y != 0.0) { used[i] = 1; used[j] = 1; }
            int cnt = 0;
            for (int i = 0; i < n; ++i) if (used[i]) { inds.push_back(i); ++cnt; }
            ks[k] = cnt;
        }
        // the contact blocks are set up whenever every contact has a support (has_blocks: the eigenchannels read
        // them); the compact products of GrLessInt / negf_transmission keep their own condition (compact_ok)
        bool has = true;
        for (int k : ks) has = has && k > 0;
        const bool ok = has && 2 * (int)inds.size() <= n;
        if (has) {
            if ((rc = setup_blocks(c, p, n_contacts, ks.data(), inds.data()))) { free_provider(p); return rc; }
            std::vector<cplx> blk((size_t)p->blk_stride);
            for (int k = 0; k < n_contacts; ++k) {
                const cplx* m = s + (size_t)k * n2;
                const int* id = p->h_inds.data() + p->inds_off[k];
                for (int a = 0; a < ks[k]; ++a)
                    for (int e = 0; e < ks[k]; ++e)
                        blk[(size_t)p->blk_off[k] + (size_t)a * ks[k] + e] = m[(size_t)id[a] * n + id[e]];
            }
            if ((rc = dev_alloc(&p->d_const_blk, blk.size())) || (rc = upload(c, p->d_const_blk, blk.data(), blk.size()))) {
                free_provider(p); return rc;
            }
            p->has_blocks = true;
            p->compact_ok = ok;
            if (!ok) {
                // blocks for the eigenchannels only: the provider keeps blk_stride = 0 (and no d_pos), as before they
                // existed -- the workspace sizes its Sigma block staging d_blk by blk_stride, and no CONST path reads
                // d_blk (formSigma's -1e-9 i S background makes every orbital part of the support: 2 n^2 per energy)
                p->blk_stride = 0;
                dev_free(p->d_pos);
            }
        }
    }
    *handle = add_provider(c, p);
    return NEGF_OK;
}

// n: the dimension the index lists live in (default: the dense system's; a layered terminal passes its layer's)
static int setup_blocks(negf_ctx* c, SigmaProvider* p, int n_contacts, const int* nc, const int* inds, int n)
{
    if (n < 0) n = c->n;
    p->n_contacts = n_contacts;
    p->nc.assign(nc, nc + n_contacts);
    p->blk_off.resize(n_contacts); p->inds_off.resize(n_contacts);
    int off = 0, ioff = 0;
    p->nc_max = 0;
    for (int k = 0; k < n_contacts; ++k) {
        if (nc[k] <= 0 || nc[k] > n) return NEGF_EINVAL;
        p->blk_off[k] = off; p->inds_off[k] = ioff;
        off += nc[k] * nc[k]; ioff += nc[k];
        p->nc_max = std::max(p->nc_max, nc[k]);
    }
    p->blk_stride = off;
    p->h_inds.assign(inds, inds + ioff);
    for (int v : p->h_inds) if (v < 0 || v >= n) return NEGF_EINVAL;
    int rc;
    if ((rc = dev_alloc(&p->d_inds, (size_t)ioff)) || (rc = dev_alloc(&p->d_nc, (size_t)n_contacts)) ||
        (rc = dev_alloc(&p->d_blk_off, (size_t)n_contacts)) || (rc = dev_alloc(&p->d_inds_off, (size_t)n_contacts)))
        return rc;
    if ((rc = upload(c, p->d_inds, p->h_inds.data(), (size_t)ioff)) ||
        (rc = upload(c, p->d_nc, p->nc.data(), (size_t)n_contacts)) ||
        (rc = upload(c, p->d_blk_off, p->blk_off.data(), (size_t)n_contacts)) ||
        (rc = upload(c, p->d_inds_off, p->inds_off.data(), (size_t)n_contacts)))
        return rc;
    // position of every orbital in each contact's index list (the small fused kernel subtracts the contact blocks while
    // it assembles); a list that names an orbital twice has no such map and keeps the scatter kernels
    std::vector<int> pos((size_t)n_contacts * n, -1);
    bool unique = true;
    for (int k = 0; k < n_contacts; ++k)
        for (int a = 0; a < nc[k]; ++a) {
            int& slot = pos[(size_t)k * n + p->h_inds[p->inds_off[k] + a]];
            if (slot >= 0) unique = false;
            slot = a;
        }
    if (unique) {
        if ((rc = dev_alloc(&p->d_pos, pos.size())) || (rc = upload(c, p->d_pos, pos.data(), pos.size()))) return rc;
    }
    return NEGF_OK;
}

// A CHAIN1D provider whose index lists live in a space of n orbitals (the dense system, or the end layer of a layered
// one): *out is owned by the caller
static int make_chain1d(negf_ctx* c, int n, int n_contacts, const int* nc, const int* inds,
                        const double* alpha, const double* Salpha, const double* beta,
                        const double* Sbeta, const double* tau, const double* Stau,
                        double eta, double conv, double relFactor, int max_iter, int force_iters,
                        SigmaProvider** out)
{
    if (n_contacts <= 0 || !nc || !inds || !alpha || !Salpha || !beta || !Sbeta || !tau || !Stau || !out)
        return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    SigmaProvider* p = new SigmaProvider();
    p->kind = SK_CHAIN1D;
    int rc = setup_blocks(c, p, n_contacts, nc, inds, n);
    if (rc) { free_provider(p); return rc; }
    const size_t tot = (size_t)p->blk_stride;
    cplx** dsts[6] = {&p->d_alpha, &p->d_Salpha, &p->d_beta, &p->d_Sbeta, &p->d_tau, &p->d_Stau};
    const double* srcs[6] = {alpha, Salpha, beta, Sbeta, tau, Stau};
    for (int k = 0; k < 6; ++k) {
        if ((rc = dev_alloc(dsts[k], tot)) ||
            (rc = upload(c, *dsts[k], reinterpret_cast<const cplx*>(srcs[k]), tot))) { free_provider(p); return rc; }
    }
    if (chain1d_lds_supported(p->nc_max)) {
        // zero-padded copies at a fixed pitch (SigmaProvider::d_lead_pad)
        const size_t mat = (size_t)CHAIN_PAD * CHAIN_PAD;
        std::vector<cplx> pad(6 * (size_t)n_contacts * mat, cmake(0.0, 0.0));
        for (int k = 0; k < 6; ++k)
            for (int q = 0; q < n_contacts; ++q) {
                const cplx* src = reinterpret_cast<const cplx*>(srcs[k]) + p->blk_off[q];
                cplx* dst = pad.data() + ((size_t)k * n_contacts + q) * mat;
                for (int i = 0; i < nc[q]; ++i) std::copy(src + (size_t)i * nc[q], src + (size_t)(i + 1) * nc[q], dst + (size_t)i * CHAIN_PAD);
            }
        if ((rc = dev_alloc(&p->d_lead_pad, pad.size())) || (rc = upload(c, p->d_lead_pad, pad.data(), pad.size()))) { free_provider(p); return rc; }
    }
    // what g(E) depends on, for the context's g(E) cache
    p->h_lead = std::make_shared<std::vector<cplx>>();
    p->h_lead->reserve(4 * tot);
    for (int k = 0; k < 4; ++k) {
        const cplx* src = reinterpret_cast<const cplx*>(srcs[k]);
        p->h_lead->insert(p->h_lead->end(), src, src + tot);
    }
    p->lead_hash = hash_words(p->h_lead->data(), p->h_lead->size() * sizeof(cplx));
    p->eta = eta; p->conv = conv; p->relFactor = relFactor; p->max_iter = max_iter;
    p->force_iters = force_iters;
    *out = p;
    return NEGF_OK;
}

int negf_sigma_chain1d(negf_ctx* c, int n_contacts, const int* nc, const int* inds,
                       const double* alpha, const double* Salpha, const double* beta,
                       const double* Sbeta, const double* tau, const double* Stau,
                       double eta, double conv, double relFactor, int max_iter, int force_iters,
                       int* handle)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (!handle) return NEGF_EINVAL;
    SigmaProvider* p = nullptr;
    int rc = make_chain1d(c, c->n, n_contacts, nc, inds, alpha, Salpha, beta, Sbeta, tau, Stau, eta, conv, relFactor,
                          max_iter, force_iters, &p);
    if (rc) return rc;
    *handle = add_provider(c, p);
    return NEGF_OK;
}

int negf_sigma_chain1d_rd(negf_ctx* c, int n_contacts, const int* nc, const int* inds,
                          const double* alpha, const double* Salpha, const double* beta,
                          const double* Sbeta, const double* tau, const double* Stau,
                          double eta, double tol, int max_steps, int force_steps, int* handle)
{
    if (!(tol >= 0.0) || max_steps < 0) return NEGF_EINVAL;
    int rc = negf_sigma_chain1d(c, n_contacts, nc, inds, alpha, Salpha, beta, Sbeta, tau, Stau, eta, tol, 1.0, max_steps,
                                force_steps, handle);
    if (rc) return rc;
    c->providers[*handle]->solver = 1;
    return NEGF_OK;
}

int negf_sigma_bethe(negf_ctx* c, int n_contacts, const int* n_atoms, const int* atom_orbs,
                     const int* n_nb, const int* nb_dirs, const double* H, const double* Slist,
                     const double* Vlist, const double* xi, double eta, double conv, double mix,
                     int max_iter, int force_iters, int* handle)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (n_contacts <= 0 || !n_atoms || !atom_orbs || !n_nb || !H || !Slist || !Vlist || !handle)
        return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    SigmaProvider* p = new SigmaProvider();
    p->kind = SK_BETHE;
    std::vector<int> nc(n_contacts);
    int total_atoms = 0;
    p->n_atoms.assign(n_atoms, n_atoms + n_contacts);
    p->atom_off.resize(n_contacts);
    for (int k = 0; k < n_contacts; ++k) {
        if (n_atoms[k] <= 0) { free_provider(p); return NEGF_EINVAL; }
        p->atom_off[k] = total_atoms;
        nc[k] = 9 * n_atoms[k];
        total_atoms += n_atoms[k];
    }
    int rc = setup_blocks(c, p, n_contacts, nc.data(), atom_orbs);
    if (rc) { free_provider(p); return rc; }
    std::vector<int> nb_off(total_atoms + 1, 0);
    for (int a = 0; a < total_atoms; ++a) {
        if (n_nb[a] < 0) { free_provider(p); return NEGF_EINVAL; }
        nb_off[a + 1] = nb_off[a] + n_nb[a];
    }
    const int total_nb = nb_off[total_atoms];
    if (total_nb > 0 && !nb_dirs) { free_provider(p); return NEGF_EINVAL; }
    if ((rc = dev_alloc(&p->d_n_atoms, (size_t)n_contacts)) || (rc = dev_alloc(&p->d_atom_off, (size_t)n_contacts)) ||
        (rc = dev_alloc(&p->d_nb_off, (size_t)total_atoms + 1)) || (rc = dev_alloc(&p->d_nb_dirs, (size_t)std::max(total_nb, 1))) ||
        (rc = dev_alloc(&p->d_H, (size_t)n_contacts * 81)) || (rc = dev_alloc(&p->d_Slist, (size_t)n_contacts * 12 * 81)) ||
        (rc = dev_alloc(&p->d_Vlist, (size_t)n_contacts * 12 * 81))) { free_provider(p); return rc; }
    if ((rc = upload(c, p->d_n_atoms, p->n_atoms.data(), (size_t)n_contacts)) ||
        (rc = upload(c, p->d_atom_off, p->atom_off.data(), (size_t)n_contacts)) ||
        (rc = upload(c, p->d_nb_off, nb_off.data(), (size_t)total_atoms + 1)) ||
        (rc = upload(c, p->d_nb_dirs, nb_dirs, (size_t)total_nb)) ||
        (rc = upload(c, p->d_H, H, (size_t)n_contacts * 81)) ||
        (rc = upload(c, p->d_Slist, Slist, (size_t)n_contacts * 12 * 81)) ||
        (rc = upload(c, p->d_Vlist, Vlist, (size_t)n_contacts * 12 * 81))) { free_provider(p); return rc; }
    if (xi) {
        const size_t n2 = (size_t)c->n * c->n;
        if ((rc = dev_alloc(&p->d_xi, n2)) ||
            (rc = upload(c, p->d_xi, reinterpret_cast<const cplx*>(xi), n2))) { free_provider(p); return rc; }
    }
    p->eta = eta; p->conv = conv; p->mix = mix; p->max_iter = max_iter; p->force_iters = force_iters;
    *handle = add_provider(c, p);
    return NEGF_OK;
}

int negf_sigma_precomputed(negf_ctx* c, int m, const double* sigma_tot, int n_contacts_c,
                           const double* sigma_c, int* handle)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (m <= 0 || !sigma_tot || !handle) return NEGF_EINVAL;
    const bool is_gamma = n_contacts_c < 0;
    if (is_gamma) { n_contacts_c = -n_contacts_c; if (!sigma_c) return NEGF_EINVAL; }
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    const size_t n2 = (size_t)c->n * c->n;
    SigmaProvider* p = new SigmaProvider();
    p->kind = SK_PRECOMPUTED; p->m_pre = m; p->n_contacts = std::max(n_contacts_c, 1);
    p->pre_nc = sigma_c ? std::max(n_contacts_c, 1) : 0;
    p->pre_is_gamma = is_gamma;
    int rc;
    if ((rc = dev_alloc(&p->d_pre_tot, n2 * m)) ||
        (rc = upload(c, p->d_pre_tot, reinterpret_cast<const cplx*>(sigma_tot), n2 * m))) { free_provider(p); return rc; }
    if (sigma_c) {
        const size_t cnt = n2 * m * p->pre_nc;
        if ((rc = dev_alloc(&p->d_pre_c, cnt)) ||
            (rc = upload(c, p->d_pre_c, reinterpret_cast<const cplx*>(sigma_c), cnt))) { free_provider(p); return rc; }
    }
    *handle = add_provider(c, p);
    return NEGF_OK;
}

int negf_sigma_free(negf_ctx* c, int handle)
{
    SigmaProvider* p = get_provider(c, handle);
    if (!p) return NEGF_EINVAL;
    (void)hipStreamSynchronize(c->stream);
    free_provider(p);
    c->providers[handle] = nullptr;
    return NEGF_OK;
}

// ------------------------------------------------------------- device variants
int negf_gr_int_dev(negf_ctx* c, int handle, int m, const double* E_dev, const double* w_dev,
                    double* out_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    const size_t n2 = (size_t)c->n * c->n;
    if ((rc = ensure_mbuffers(c, m, p->n_contacts))) return rc;
    if (small_path(c, p) && m > 0) {
        // n <= 96: assemble + inverse + weighted sum in one kernel (plus the reduction of the workgroups' partial sums);
        // no n x n work area in HBM at all.  Grids above SMALL_CHUNK points go through in chunks (the Sigma blocks of a
        // block provider are staged per chunk); chunk sums are added in order.
        const cplx* E = reinterpret_cast<const cplx*>(E_dev);
        const cplx* w = reinterpret_cast<const cplx*>(w_dev);
        cplx* out = reinterpret_cast<cplx*>(out_dev);
        constexpr int SMALL_CHUNK = 16384;
        const bool blocks = p->kind == SK_CHAIN1D || p->kind == SK_BETHE;
        const int chunk = std::min(m, SMALL_CHUNK);
        if (blocks && (rc = ensure_cap(c, c->d_blk, (size_t)chunk * p->blk_stride))) return rc;
        if ((rc = ensure_cap(c, c->d_small_part, (size_t)small_fused_grid(c->n, chunk) * n2 + (m > chunk ? n2 : 0)))) return rc;
        cplx* chunk_sum = c->d_small_part + (size_t)small_fused_grid(c->n, chunk) * n2;   // (only with several chunks)
        for (int m0 = 0; m0 < m; m0 += chunk) {
            const int nb = std::min(chunk, m - m0);
            if (blocks && (rc = run_sigma_blocks(c, p, nb, E + m0, c->d_iters + (size_t)m0 * p->n_contacts,
                                                 c->d_conv + (size_t)m0 * p->n_contacts, m0))) return rc;
            ProfScope ps(c, "small");
            SmallFusedArgs a = small_args(c, p, m0, nb, E);
            a.w = w + m0; a.partial = c->d_small_part; a.out = m0 == 0 ? out : chunk_sum;
            launch_small_fused(c->stream, a);
            if (m0 > 0) launch_cadd(c->stream, n2, out, chunk_sum, out);
            negf_count_flops(8.0 * c->n * (double)c->n * c->n * nb, 0.0);
        }
        return close_call(c, m);
    }
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    const cplx* w = reinterpret_cast<const cplx*>(w_dev);
    cplx* out = reinterpret_cast<cplx*>(out_dev);
    return dense_batches(c, p, m, clear_first(c, out, n2 * sizeof(cplx)), [&](int m0, int nb) {
        bool perm;
        if (int e = run_inverse_for_sum(c, p, m0, nb, E, &perm)) return e;
        ProfScope ps(c, "accumulate");
        if (perm) launch_accumulate_perm(c->stream, c->n, nb, w + m0, c->W1, c->d_ipiv, c->d_info + m0, out, c->W2);
        else launch_accumulate(c->stream, (int)n2, nb, w + m0, c->G, out, c->W2);
        return NEGF_OK;
    });
}

// c->W1 = G D G^H of the batch in c->G for a Hermitian D [nb] (stride sD; Gamma_c, or the dephased coupling): on the K
// columns idx of G (D is K x K; G[:, idx] and X live in the free buffer W2, 2 n K <= n^2) or, idx null, dense (D n x n).
// X = (. D)^H -- the first product stores its result conjugate-transposed -- and W1 = . X ( = G D^H G^H), upper block
// tiles computed, lower ones mirrored: both products read their second operand in the plain form (k_zgemm.hip: the
// operand conjugate-transposed on the fly costs the L2 twice the requests).
static void launch_g_d_gh(negf_ctx* c, int nb, int K, const int* idx, const cplx* D, size_t sD)
{
    const int n = c->n;
    const size_t n2 = (size_t)n * n;
    if (!idx) {
        launch_zgemm(c->stream, n, n, n, nb, c->G, n, n2, D, n, sD, 4, c->W2, n, n2);
        launch_zgemm(c->stream, n, n, n, nb, c->G, n, n2, c->W2, n, n2, 2, c->W1, n, n2);
        return;
    }
    cplx* Gc = c->W2;                              // [nb][n x K]
    cplx* X = c->W2 + (size_t)n * K;               // [nb][n x K]
    launch_gather_block(c->stream, n, n, K, nb, c->G, n2, nullptr, idx, Gc, n2);
    launch_zgemm(c->stream, n, K, K, nb, Gc, K, n2, D, K, sD, 4, X, n, n2);
    launch_zgemm(c->stream, n, n, K, nb, Gc, K, n2, X, n, n2, 2, c->W1, n, n2);
}

// A_c = G Gamma_c G^H for the batch [m0, m0 + nb) -> c->W1 (Hermitian unless the caller handed in its own coupling
// matrices); c->W2 is free again on return.  Shared by GrLessInt and the local transmission.
static int run_gless_products(negf_ctx* c, SigmaProvider* p, int contact, int m0, int nb, const cplx* E)
{
    int rc;
    const size_t n2 = (size_t)c->n * c->n;
    const int n = c->n;
    if ((rc = run_assemble_inverse(c, p, m0, nb, E))) return rc;
    if (compact_available(c, p)) {
        // G Gamma G^H = (G[:, I] Gamma_II) G[:, I]^H
        GammaSmall g;
        { ProfScope ps(c, "gamma"); if ((rc = run_gamma_small(c, p, contact, nb, 0, &g))) return rc; }
        ProfScope ps(c, "zgemm");
        launch_g_d_gh(c, nb, g.K, g.idx, g.mat, g.stride);
        return NEGF_OK;
    }
    size_t gs = 0;
    const cplx* gam = nullptr;
    { ProfScope ps(c, "gamma"); if ((rc = run_gamma(c, p, contact, m0, nb, c->W1, c->W2, &gam, &gs))) return rc; }
    ProfScope ps(c, "zgemm");
    // G Gamma G^H (integrate.py:81).  Gamma = i (Sigma - Sigma^H) is Hermitian, element by element, and so is the result.
    if (!(p->kind == SK_PRECOMPUTED && p->pre_is_gamma)) { launch_g_d_gh(c, nb, n, nullptr, gam, gs); return NEGF_OK; }
    // (coupling matrices handed in by the caller need not be Hermitian: X = G Gamma, then the full product X G^H)
    launch_zgemm(c->stream, n, n, n, nb, c->G, n, n2, gam, n, gs, 0, c->W2, n, n2);
    launch_zgemm(c->stream, n, n, n, nb, c->W2, n, n2, c->G, n, n2, 1, c->W1, n, n2);
    return NEGF_OK;
}

// sum_m w_m G Gamma_c G^H over the energies E[0..m) (device pointers).  nseg == 0: one sum into out [n*n]; nseg > 0: the
// energies are nseg consecutive segments ending at seg_end[s] (host array) and out [nseg][n*n] receives one sum each.
static int gless_core(negf_ctx* c, SigmaProvider* p, int contact, int m, const cplx* E, const cplx* w, cplx* out,
                      int nseg, const int* seg_end)
{
    const size_t n2 = (size_t)c->n * c->n;
    return dense_batches(c, p, m, clear_first(c, out, (size_t)std::max(nseg, 1) * n2 * sizeof(cplx)), [&](int m0, int nb) {
        if (int e = run_gless_products(c, p, contact, m0, nb, E)) return e;
        const cplx* X = c->W1;
        ProfScope ps(c, "accumulate");
        if (nseg == 0) { launch_accumulate(c->stream, (int)n2, nb, w + m0, X, out, c->W2); return NEGF_OK; }
        const SegShares sh = batch_shares(nseg, seg_end, m0, nb);
        for (size_t k = 0; k < sh.slot.size(); ++k)
            launch_accumulate(c->stream, (int)n2, sh.hi[k] - sh.lo[k], w + m0 + sh.lo[k], X + (size_t)sh.lo[k] * n2, out + (size_t)sh.slot[k] * n2, c->W2);
        return NEGF_OK;
    });
}

int negf_gless_int_dev(negf_ctx* c, int handle, int ind, int m, const double* E_dev,
                       const double* w_dev, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = open_call(c, handle, m, &p, ind, &contact);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    return gless_core(c, p, contact, m, reinterpret_cast<const cplx*>(E_dev), reinterpret_cast<const cplx*>(w_dev),
                      reinterpret_cast<cplx*>(out_dev), 0, nullptr);
}

int negf_transmission_dev(negf_ctx* c, int handle, int contact_L, int contact_R, int spin_mode,
                          int m, const double* E_dev, double* T_dev, double* Tspin_dev)
{
    SigmaProvider* p;
    int cL, cR;
    int rc = open_call(c, handle, m, &p, contact_L, &cL, contact_R, &cR);
    if (rc) return rc;
    if (!T_dev || (m > 0 && !E_dev)) return NEGF_EINVAL;
    if (spin_mode != NEGF_SPIN_RESTRICTED && spin_mode != NEGF_SPIN_BLOCK) return NEGF_EINVAL;
    if (spin_mode == NEGF_SPIN_BLOCK && (!Tspin_dev || (c->n & 1))) return NEGF_EINVAL;
    const int n = c->n;
    const size_t n2 = (size_t)n * n;
    if ((rc = ensure_mbuffers(c, m, p->n_contacts))) return rc;
    // two extra n x n work areas per energy for Gamma_L / Gamma_R: reuse T1/T2 for
    // the Gammas and carve the product temporaries out of a second workspace half
    c->transmission_seen = true;
    if ((rc = ensure_workspace(c, m, p->blk_stride, 2))) return rc;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    // process with half the allocated batch so that [0,half) holds this sweep's
    // matrices and [half, 2*half) is free scratch in each of A/T1/T2
    const int half = std::max(1, c->batch / 2);
    for (int m0 = 0; m0 < m; m0 += half) {
        const int nb = std::min(half, m - m0);
        if ((rc = run_assemble_inverse(c, p, m0, nb, E))) return rc;
        if (spin_mode == NEGF_SPIN_RESTRICTED && compact_available(c, p)) {
            // T = Re sum_ij Y_ij conj(G_ij), Y = Gamma_L G Gamma_R: only G[I_L, I_R] enters
            GammaSmall gL, gR;
            {
                ProfScope ps(c, "gamma");
                if ((rc = run_gamma_small(c, p, cL, nb, 0, &gL))) return rc;
                if ((rc = run_gamma_small(c, p, cR, nb, 1, &gR))) return rc;
            }
            const size_t kk = (size_t)gL.K * gR.K;            // 3 kk <= n^2
            cplx* Glr = c->W2; cplx* Xs = c->W2 + kk; cplx* Ys = c->W2 + 2 * kk;
            {
                ProfScope ps(c, "zgemm");
                launch_gather_block(c->stream, n, gL.K, gR.K, nb, c->G, n2, gL.idx, gR.idx, Glr, n2);
                launch_zgemm(c->stream, gL.K, gR.K, gL.K, nb, gL.mat, gL.K, gL.stride, Glr, gR.K, n2, 0, Xs, gR.K, n2);
                launch_zgemm(c->stream, gL.K, gR.K, gR.K, nb, Xs, gR.K, n2, gR.mat, gR.K, gR.stride, 0, Ys, gR.K, n2);
            }
            ProfScope ps(c, "trace");
            launch_trace_dot(c->stream, gL.K, gR.K, nb, Ys, gR.K, n2, Glr, gR.K, n2, T_dev + m0, 1);
            continue;
        }
        cplx* G = c->G;
        const cplx* gamL = nullptr;           // [nb] (or one shared matrix)
        const cplx* gamR = nullptr;
        cplx* X = c->W2;                      // [nb]
        cplx* Y = c->G + n2 * half;           // [nb] upper half of the buffer holding G (unused by this sweep)
        size_t gsL = 0, gsR = 0;
        {
            ProfScope ps(c, "gamma");
            // W2 doubles as run_gamma's scratch -> build both Gammas before X is live
            if ((rc = run_gamma(c, p, cL, m0, nb, c->W1, c->W2, &gamL, &gsL))) return rc;
            if ((rc = run_gamma(c, p, cR, m0, nb, c->W1 + n2 * half, c->W2, &gamR, &gsR))) return rc;
        }
        if (spin_mode == NEGF_SPIN_RESTRICTED) {
            {
                ProfScope ps(c, "zgemm");
                // T = Re Tr[Gamma_L G Gamma_R G^H]  (transport.py:156-157) as  X = (G Gamma_R)^H ;  M = G X -- Hermitian,
                // as Gamma_R is: upper block tiles only (launch_zgemm opB bit 2) -- ;  T = Re sum Gamma_L,ij conj(M_ij)
                // ( = Re Tr[Gamma_L M], M_ji = conj(M_ij)): one and a half dense products instead of two
                // (explicit Gamma matrices handed in by the caller -- negf_sigma_precomputed with gammas, the
                //  reference's _transmission_kernel_restricted(E, F, S, sigma, gamma1, gamma2) -- need not be
                //  Hermitian: M is then computed in full, opB = 1, and T = Re Tr[Gamma_L M] = Re sum Gamma_L,ij M_ji
                //  is taken with M^H: sum Re(Gamma_L,ij conj(M^H_ij)))
                const bool herm_ok = !(p->kind == SK_PRECOMPUTED && p->pre_is_gamma);
                if (herm_ok) {
                    // X = (G Gamma_R)^H stored by the first product, M = G X: both second operands in the plain form
                    launch_zgemm(c->stream, n, n, n, nb, G, n, n2, gamR, n, gsR, 4, X, n, n2);
                    launch_zgemm(c->stream, n, n, n, nb, G, n, n2, X, n, n2, 2, Y, n, n2);           // Y = M = G Gamma_R G^H
                } else {
                    launch_zgemm(c->stream, n, n, n, nb, G, n, n2, gamR, n, gsR, 0, X, n, n2);
                    launch_zgemm(c->stream, n, n, n, nb, G, n, n2, X, n, n2, 1, Y, n, n2);           // Y = G X^H = M^H
                }
            }
            ProfScope ps(c, "trace");
            launch_trace_dot(c->stream, n, n, nb, gamL, n, gsL, Y, n, n2, T_dev + m0, 1);
        } else {
            const int h = n / 2;
            // blocks [uu, ud, du, dd]: G rows/cols offsets; Gamma_L blocks [uu,uu,dd,dd];
            // Gamma_R blocks [uu,dd,uu,dd]; Ga_k = (G^H)[R,C] = conj(G[C,R])^T  (transport.py:166-177)
            const int gr[4] = {0, 0, h, h}, gc[4] = {0, h, 0, h};
            const int l_off[4] = {0, 0, h, h}, r_off[4] = {0, h, 0, h};
            for (int k = 0; k < 4; ++k) {
                const cplx* Gk = G + (size_t)gr[k] * n + gc[k];
                const cplx* GLk = gamL + (size_t)l_off[k] * n + l_off[k];
                const cplx* GRk = gamR + (size_t)r_off[k] * n + r_off[k];
                // trace pairs X_k[i][j] with conj(G[C0+i][R0+j])
                const cplx* Gpair = G + (size_t)gc[k] * n + gr[k];
                {
                    ProfScope ps(c, "zgemm");
                    launch_zgemm(c->stream, h, h, h, nb, GLk, n, gsL, Gk, n, n2, 0, X, h, n2);
                    launch_zgemm(c->stream, h, h, h, nb, X, h, n2, GRk, n, gsR, 0, Y, h, n2);
                }
                ProfScope ps(c, "trace");
                launch_trace_dot(c->stream, h, h, nb, Y, h, n2, Gpair, n, n2, Tspin_dev + (size_t)m0 * 4 + k, 4);
            }
        }
    }
    return close_call(c, m);
}

int negf_sync(negf_ctx* c)
{
    if (!c) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    return NEGF_OK;
}

int negf_last_info(negf_ctx* c, int m, int* info)
{
    if (!c || !info || m < 0 || m > c->m_cap) return NEGF_EINVAL;
    return download(c, info, c->d_info, (size_t)m);
}

int negf_last_iters(negf_ctx* c, int handle, int m, int* iters, int* converged)
{
    SigmaProvider* p = get_provider(c, handle);
    if (!c || !p || m < 0 || m > c->m_cap) return NEGF_EINVAL;
    if ((p->kind == SK_CHAIN1D || p->kind == SK_BETHE) && p->n_contacts > c->contacts_cap) return NEGF_EINVAL;
    return fetch_iters(c, p, m, iters, converged);
}

// --------------------------------------------------------------- host variants
// The host-pointer entry points stage through ONE pinned buffer of the context: [E | w] go up with two asynchronous
// copies and no synchronisation (the buffer is ours; the call's final synchronisation covers them), the result and the
// per-energy info come down into [out | info] and are handed over after ONE synchronisation.  (Pageable copies with a
// synchronisation each made a 2-point integral of a 60-orbital system cost 0.5 ms of host time: bench.py --config scf.)
// THE layout of that buffer for a grid of m energies: [E | w | result | extra | info] -- byte offsets of the parts and
// the size of the whole.  `extra` is whatever else a call brings back behind its result (negf_gr_int_refine's level tables).
struct PinLayout {
    size_t E = 0, w, result, extra, info, bytes;
    PinLayout(int m, size_t result_bytes, size_t extra_bytes = 0)
    {
        const size_t gb = (size_t)m * sizeof(cplx);
        w = gb; result = 2 * gb; extra = result + result_bytes; info = extra + extra_bytes;
        bytes = info + (size_t)m * sizeof(int) + 64;
    }
};

// the device side of a staged call as the *_dev forms take it: the grid, the weights, the n x n accumulator
static double* dev_E(negf_ctx* c) { return reinterpret_cast<double*>(c->d_E); }
static double* dev_w(negf_ctx* c) { return reinterpret_cast<double*>(c->d_w); }
static double* dev_acc(negf_ctx* c) { return reinterpret_cast<double*>(c->d_acc); }

// the grid goes up; the pinned buffer has room for a result of result_bytes (at least one n x n matrix) + extra_bytes
static int stage_grid(negf_ctx* c, int m, int contacts, const double* E, const double* w, size_t result_bytes = 0,
                      size_t extra_bytes = 0)
{
    int rc = ensure_mbuffers(c, m, contacts);
    if (rc) return rc;
    const PinLayout L(m, std::max(result_bytes, (size_t)c->n * c->n * sizeof(cplx)), extra_bytes);
    const size_t gb = (size_t)m * sizeof(cplx);
    if ((rc = ensure_pinned(c, L.bytes))) return rc;
    if (E && m > 0) {
        c->h_E_valid = false;
        std::memcpy(c->h_pin + L.E, E, gb);
        NEGF_HIP_CHECK(hipMemcpyAsync(c->d_E, c->h_pin + L.E, gb, hipMemcpyHostToDevice, c->stream));
        const cplx* Eh = reinterpret_cast<const cplx*>(E);
        c->h_E.assign(Eh, Eh + m);
        c->h_E_valid = true;
    }
    if (w && m > 0) {
        std::memcpy(c->h_pin + L.w, w, gb);
        NEGF_HIP_CHECK(hipMemcpyAsync(c->d_w, c->h_pin + L.w, gb, hipMemcpyHostToDevice, c->stream));
    }
    return NEGF_OK;
}

// result (`bytes` from d_src) and per-energy info back to the caller: two asynchronous copies into the pinned buffer,
// one synchronisation; returns NEGF_ESINGULAR when an energy reported a zero pivot
static int fetch_result_and_info(negf_ctx* c, int m, const void* d_src, size_t bytes, void* out_host, int* info_host,
                                 size_t extra_bytes = 0)
{
    const PinLayout L(m, bytes, extra_bytes);
    unsigned char* pout = c->h_pin + L.result;
    const int* pinfo = reinterpret_cast<const int*>(c->h_pin + L.info);
    NEGF_HIP_CHECK(hipMemcpyAsync(pout, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    if (m > 0) NEGF_HIP_CHECK(hipMemcpyAsync(c->h_pin + L.info, c->d_info, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    { const int wrc = wait_stream(c); if (wrc) return wrc; }
    copy_bytes(out_host, pout, bytes);
    int rc = NEGF_OK;
    for (int i = 0; i < m; ++i) { if (info_host) info_host[i] = pinfo[i]; if (pinfo[i] != 0) rc = NEGF_ESINGULAR; }
    return rc;
}

// The same way back for results too large to pin (G(E), psi, per-energy tables): every output [count] comes down with a
// pageable copy and a wait of its own, in the order given, then the info (reduce_info, one more copy and wait).
extern "C++" struct HostOut {
    void* dst; const void* src; size_t bytes;
    template <typename T>
    HostOut(T* host_dst, const T* dev_src, size_t count) : dst(host_dst), src(dev_src), bytes(count * sizeof(T)) {}
};
static int fetch_pageable(negf_ctx* c, int m, std::initializer_list<HostOut> outs, int* info_host)
{
    for (const HostOut& o : outs)
        if (int rc = download(c, static_cast<unsigned char*>(o.dst), static_cast<const unsigned char*>(o.src), o.bytes)) return rc;
    return reduce_info(c, m, info_host);
}

// real weights w [m] of a bond integral: they ride in the [w] part of the pinned buffer and of d_w (m doubles of their m
// complex values); stage_grid has run with a result of result_bytes
static int stage_real_weights(negf_ctx* c, int m, const double* w, size_t result_bytes)
{
    if (m <= 0) return NEGF_OK;
    unsigned char* pw = c->h_pin + PinLayout(m, result_bytes).w;
    std::memcpy(pw, w, (size_t)m * sizeof(double));
    NEGF_HIP_CHECK(hipMemcpyAsync(c->d_w, pw, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return NEGF_OK;
}

// The host form of an integral into ONE n x n matrix -- GrInt, GrLessInt, either with n_probes probes --: grid and weights
// staged, dev(E, w, acc) run on the staged device pointers, matrix and info back through the pinned buffer
extern "C++" template <class Dev>
static int host_integral(negf_ctx* c, int handle, int n_probes, int m, const double* E, const double* w, double* out, int* info, Dev&& dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!probes_count_ok(p, n_probes) || !out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    if ((rc = stage_grid(c, m, p->n_contacts, E, w)) || (rc = dev(dev_E(c), dev_w(c), dev_acc(c)))) return rc;
    return fetch_result_and_info(c, m, c->d_acc, (size_t)c->n * c->n * sizeof(cplx), out, info);
}

int negf_gr_int(negf_ctx* c, int handle, int m, const double* E, const double* w, double* out, int* info)
{
    return host_integral(c, handle, 0, m, E, w, out, info,
                         [&](double* Ed, double* wd, double* acc) { return negf_gr_int_dev(c, handle, m, Ed, wd, acc); });
}

// Several integrals of the same system in ONE pass: the energies are nseg consecutive segments (seg_end[s] = index one
// past the last point of segment s) and out receives one n x n sum per segment.  This is how the adaptive integrations
// (nested ANT levels 2, 6, 18, 54 ... of density.py:211-273; the doubling real-axis grids of :438-484) are served: the
// levels a refinement is going to visit are evaluated together -- a level of 2 ... 36 points alone in a launch is pure
// latency on this chip -- and handed back level by level.
static int check_segments(int m, int nseg, const int* seg_end)
{
    if (nseg <= 0 || !seg_end) return NEGF_EINVAL;
    for (int sg = 0, prev = 0; sg < nseg; ++sg) { if (seg_end[sg] < prev || seg_end[sg] > m) return NEGF_EINVAL; prev = seg_end[sg]; }
    return seg_end[nseg - 1] == m ? NEGF_OK : NEGF_EINVAL;
}

// sum_m w_m G(E_m) per segment, everything on the device: Ed, wd [m], out [nseg][n*n]; seg_end is a host array
static int gr_seg_core(negf_ctx* c, SigmaProvider* p, int m, const cplx* Ed, const cplx* wd, int nseg, const int* seg_end,
                       cplx* out)
{
    int rc;
    const size_t n2 = (size_t)c->n * c->n;
    if (m > 0 && small_path(c, p) && m <= 4096) {
        const bool blocks = p->kind == SK_CHAIN1D || p->kind == SK_BETHE;
        if (blocks && (rc = ensure_cap(c, c->d_blk, (size_t)m * p->blk_stride))) return rc;
        if ((rc = ensure_cap(c, c->d_small_part, (size_t)m * n2))) return rc;
        if (blocks && (rc = run_sigma_blocks(c, p, m, Ed, c->d_iters, c->d_conv, 0))) return rc;
        ProfScope ps(c, "small");
        SmallFusedArgs a = small_args(c, p, 0, m, Ed);
        a.w = wd; a.partial = c->d_small_part; a.out = out; a.nseg = nseg; a.seg_end = seg_end;
        launch_small_fused(c->stream, a);
        negf_count_flops(8.0 * c->n * (double)c->n * c->n * m, 0.0);
        return close_call(c, m);
    }
    return dense_batches(c, p, m, clear_first(c, out, (size_t)nseg * n2 * sizeof(cplx)), [&](int m0, int nb) {
        bool perm;
        if (int e = run_inverse_for_sum(c, p, m0, nb, Ed, &perm)) return e;
        ProfScope ps(c, "accumulate");
        // every segment's share of this batch in ONE launch pair (a joint arc + tail probe: 12 segments = 24 launches
        // of a few microseconds each behind a millisecond of inverse)
        const SegShares sh = batch_shares(nseg, seg_end, m0, nb);
        if (launch_accumulate_ranges(c->stream, c->n, perm, wd + m0, perm ? c->W1 : c->G, c->d_ipiv, c->d_info + m0,
                                     (int)sh.slot.size(), sh.lo.data(), sh.hi.data(), sh.slot.data(), out, c->W2)) return NEGF_OK;
        for (size_t k = 0; k < sh.slot.size(); ++k) {
            const int lo = sh.lo[k], cnt = sh.hi[k] - lo;
            cplx* dst = out + (size_t)sh.slot[k] * n2;
            if (perm)
                launch_accumulate_perm(c->stream, c->n, cnt, wd + m0 + lo, c->W1 + (size_t)lo * n2,
                                       c->d_ipiv + (size_t)lo * 2 * c->n, c->d_info + m0 + lo, dst, c->W2);
            else
                launch_accumulate(c->stream, (int)n2, cnt, wd + m0 + lo, c->G + (size_t)lo * n2, dst, c->W2);
        }
        return NEGF_OK;
    });
}

int negf_gr_int_seg_dev(negf_ctx* c, int handle, int m, const double* E_dev, const double* w_dev, int nseg,
                        const int* seg_end, double* out_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev)) || check_segments(m, nseg, seg_end)) return NEGF_EINVAL;
    if ((rc = ensure_mbuffers(c, m, p->n_contacts))) return rc;
    return gr_seg_core(c, p, m, reinterpret_cast<const cplx*>(E_dev), reinterpret_cast<const cplx*>(w_dev), nseg, seg_end,
                       reinterpret_cast<cplx*>(out_dev));
}

// negf_gr_int_seg (ind null) and negf_gless_int_seg: [nseg][n*n] sums on the device, then one download of all of them and
// the info, one synchronisation
static int host_seg_int(negf_ctx* c, int handle, const int* ind, int m, const double* E, const double* w, int nseg,
                        const int* seg_end, double* out, int* info)
{
    SigmaProvider* p;
    int contact = -1;
    int rc = open_call(c, handle, m, &p, ind ? *ind : 0, ind ? &contact : nullptr);
    if (rc) return rc;
    if (!out || (m > 0 && (!E || !w)) || check_segments(m, nseg, seg_end)) return NEGF_EINVAL;
    const size_t cnt = (size_t)nseg * c->n * c->n;
    if ((rc = stage_grid(c, m, p->n_contacts, E, w, cnt * sizeof(cplx))) || (rc = ensure_cap(c, c->d_seg_out, cnt))) return rc;
    if ((rc = ind ? gless_core(c, p, contact, m, c->d_E, c->d_w, c->d_seg_out, nseg, seg_end)
                  : gr_seg_core(c, p, m, c->d_E, c->d_w, nseg, seg_end, c->d_seg_out))) return rc;
    return fetch_result_and_info(c, m, c->d_seg_out, cnt * sizeof(cplx), out, info);
}

int negf_gr_int_seg(negf_ctx* c, int handle, int m, const double* E, const double* w, int nseg,
                    const int* seg_end, double* out, int* info)
{
    return host_seg_int(c, handle, nullptr, m, E, w, nseg, seg_end, out, info);
}

// Adaptive nested quadrature with the refinement ON THE DEVICE (integratePointsAdaptiveANT, density.py:211-273): the m energies
// are the NEW nodes of consecutive levels of nint integrations (nlev[k] levels each, seg_end as in negf_gr_int_seg over all
// sum(nlev) levels, integral after integral); ratio[s] is the nested-weight ratio of level s -- NaN for the first level of an
// integration, which then starts from that level's sum; otherwise the integration continues from P_in[k].  One pass evaluates
// every level's sum, refine_levels_kernel (n > 512: one refine_wide_kernel launch per level) runs the reference's update and
// stopping test level by level, and only the result comes back: P_out [nint][n][n] (the value at the converged level, or after the last level), level_out [nint] (index of the
// converged level within the call, -1: not converged, continue with P_out as P_in), maxdp_out [sum(nlev)].  Saves the host the
// level sums (12 x n^2 per Fermi probe), the five numpy passes per level over them, and their download.
int negf_gr_int_refine(negf_ctx* c, int handle, int m, const double* E, const double* w, int nint, const int* nlev,
                       const int* seg_end, const double* ratio, double tol, const double* P_in, double* P_out,
                       int* level_out, double* maxdp_out, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!P_out || !level_out || !maxdp_out || !nlev || !ratio || nint <= 0 || nint > REF_MAX_INTS || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    int nseg = 0;
    std::vector<int> first(nint + 1, 0);
    for (int k = 0; k < nint; ++k) { if (nlev[k] <= 0) return NEGF_EINVAL; nseg += nlev[k]; first[k + 1] = nseg; }
    if (nseg > REF_MAX_LEVELS || check_segments(m, nseg, seg_end)) return NEGF_EINVAL;
    for (int k = 0; k < nint; ++k) {
        for (int s = first[k] + 1; s < first[k + 1]; ++s) if (ratio[s] != ratio[s]) return NEGF_EINVAL;      // only a first level starts an integration
        if (ratio[first[k]] == ratio[first[k]] && !P_in) return NEGF_EINVAL;                                  // a continued one needs its running value
    }
    const size_t n2 = (size_t)c->n * c->n;
    const size_t pb = (size_t)nint * n2 * sizeof(cplx);
    const size_t meta_b = (size_t)REF_MAX_LEVELS * 24 + (size_t)(2 * REF_MAX_INTS + 1 + REF_MAX_LEVELS) * 4;
    // pinned layout: the result is P (in, then out), the extra part ratio | maxdp | first | level
    const PinLayout L(m, pb, meta_b);
    if ((rc = stage_grid(c, m, p->n_contacts, E, w, pb, meta_b))) return rc;
    if ((rc = ensure_cap(c, c->d_seg_out, (size_t)nseg * n2)) || (rc = ensure_cap(c, c->d_ref_P, (size_t)nint * n2))) return rc;
    if (!c->d_ref_meta && (rc = dev_alloc(&c->d_ref_meta, meta_b))) return rc;
    unsigned char* pP = c->h_pin + L.result;
    double* h_ratio = reinterpret_cast<double*>(c->h_pin + L.extra);
    double* h_maxdp = h_ratio + REF_MAX_LEVELS;
    int* h_first = reinterpret_cast<int*>(h_maxdp + 2 * REF_MAX_LEVELS);          // (the host side mirrors the device layout)
    int* h_level = h_first + REF_MAX_INTS + 1;
    double* d_ratio = reinterpret_cast<double*>(c->d_ref_meta);
    double* d_maxdp = d_ratio + REF_MAX_LEVELS;
    unsigned long long* d_maxbits = reinterpret_cast<unsigned long long*>(d_maxdp + REF_MAX_LEVELS);
    int* d_first = reinterpret_cast<int*>(d_maxbits + REF_MAX_LEVELS);
    int* d_level = d_first + REF_MAX_INTS + 1;
    int* d_nanflag = d_level + REF_MAX_INTS;
    std::memcpy(h_ratio, ratio, (size_t)nseg * sizeof(double));
    std::memcpy(h_first, first.data(), (size_t)(nint + 1) * sizeof(int));
    NEGF_HIP_CHECK(hipMemcpyAsync(d_ratio, h_ratio, (size_t)nseg * sizeof(double), hipMemcpyHostToDevice, c->stream));
    NEGF_HIP_CHECK(hipMemcpyAsync(d_first, h_first, (size_t)(nint + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < nint; ++k)
        if (ratio[first[k]] == ratio[first[k]]) {                // continued: its running value goes up
            std::memcpy(pP + (size_t)k * n2 * sizeof(cplx), P_in + (size_t)k * n2 * 2, n2 * sizeof(cplx));
            NEGF_HIP_CHECK(hipMemcpyAsync(c->d_ref_P + (size_t)k * n2, pP + (size_t)k * n2 * sizeof(cplx), n2 * sizeof(cplx),
                                          hipMemcpyHostToDevice, c->stream));
        }
    if ((rc = gr_seg_core(c, p, m, c->d_E, c->d_w, nseg, seg_end, c->d_seg_out))) return rc;
    {
        ProfScope ps(c, "accumulate");
        if (c->n <= REF_MAX_N) {
            launch_refine_levels(c->stream, (int)n2, nint, c->d_seg_out, d_first, d_ratio, tol, c->d_ref_P, d_level, d_maxdp);
        } else {
            // one launch pair per level, queued without a host round trip (refine_wide_kernel)
            NEGF_HIP_CHECK(hipMemsetAsync(d_maxbits, 0, (size_t)nseg * sizeof(unsigned long long), c->stream));
            NEGF_HIP_CHECK(hipMemsetAsync(d_nanflag, 0, (size_t)nseg * sizeof(int), c->stream));
            NEGF_HIP_CHECK(hipMemsetAsync(d_level, 0xFF, (size_t)nint * sizeof(int), c->stream));            // -1: not converged
            NEGF_HIP_CHECK(hipMemsetAsync(d_maxdp, 0xFF, (size_t)nseg * sizeof(double), c->stream));         // all-ones: a NaN
            for (int k = 0; k < nint; ++k)
                for (int s = first[k]; s < first[k + 1]; ++s) {
                    cplx* Pk = c->d_ref_P + (size_t)k * n2;
                    const cplx* inc = c->d_seg_out + (size_t)s * n2;
                    if (ratio[s] != ratio[s])
                        NEGF_HIP_CHECK(hipMemcpyAsync(Pk, inc, n2 * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream));
                    else
                        launch_refine_level_wide(c->stream, (int)n2, inc, ratio[s], Pk, s - first[k], tol, d_level + k,
                                                 d_maxbits + s, d_nanflag + s, d_maxdp + s);
                }
        }
    }
    NEGF_HIP_CHECK(hipGetLastError());
    NEGF_HIP_CHECK(hipMemcpyAsync(h_maxdp, d_maxdp, (size_t)nseg * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NEGF_HIP_CHECK(hipMemcpyAsync(h_level, d_level, (size_t)nint * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    rc = fetch_result_and_info(c, m, c->d_ref_P, pb, P_out, info, meta_b);
    if (rc < 0) return rc;
    std::memcpy(maxdp_out, h_maxdp, (size_t)nseg * sizeof(double));
    std::memcpy(level_out, h_level, (size_t)nint * sizeof(int));
    return rc;
}

// the same for GrLessInt (the adaptive bias-window integral, densityGrid, density.py:605-658)
int negf_gless_int_seg(negf_ctx* c, int handle, int ind, int m, const double* E, const double* w, int nseg,
                       const int* seg_end, double* out, int* info)
{
    return host_seg_int(c, handle, &ind, m, E, w, nseg, seg_end, out, info);
}

int negf_gless_int_seg_dev(negf_ctx* c, int handle, int ind, int m, const double* E_dev, const double* w_dev, int nseg,
                           const int* seg_end, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = open_call(c, handle, m, &p, ind, &contact);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev)) || check_segments(m, nseg, seg_end)) return NEGF_EINVAL;
    return gless_core(c, p, contact, m, reinterpret_cast<const cplx*>(E_dev), reinterpret_cast<const cplx*>(w_dev),
                      reinterpret_cast<cplx*>(out_dev), nseg, seg_end);
}

int negf_gless_int(negf_ctx* c, int handle, int ind, int m, const double* E, const double* w, double* out, int* info)
{
    return host_integral(c, handle, 0, m, E, w, out, info,
                         [&](double* Ed, double* wd, double* acc) { return negf_gless_int_dev(c, handle, ind, m, Ed, wd, acc); });
}

int negf_gr_batch(negf_ctx* c, int handle, int m, const double* E, double* G_out, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (m > 0 && (!E || !G_out)) return NEGF_EINVAL;
    const size_t n2 = (size_t)c->n * c->n;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr))) return rc;
    rc = dense_batches(c, p, m, [&](int m0, int nb) {
        if (int e = run_assemble_inverse(c, p, m0, nb, c->d_E)) return e;
        return download(c, reinterpret_cast<cplx*>(G_out) + n2 * m0, c->G, n2 * nb);
    });
    return rc ? rc : reduce_info(c, m, info);      // (every batch came down as it was ready: nothing is left but the info)
}

int negf_transmission(negf_ctx* c, int handle, int contact_L, int contact_R, int spin_mode, int m,
                      const double* E, double* T, double* Tspin, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (m > 0 && (!E || !T)) return NEGF_EINVAL;
    if (spin_mode == NEGF_SPIN_BLOCK && !Tspin) return NEGF_EINVAL;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr))) return rc;
    double* dT = c->d_scal;                 // [m]
    double* dTs = c->d_scal + c->m_cap;     // [m][4]
    if ((rc = negf_transmission_dev(c, handle, contact_L, contact_R, spin_mode, m, dev_E(c), dT, dTs))) return rc;
    if (spin_mode != NEGF_SPIN_BLOCK) return fetch_pageable(c, m, {{T, dT, (size_t)m}}, info);
    rc = fetch_pageable(c, m, {{Tspin, dTs, (size_t)m * 4}}, info);
    // total = sum of the four components in order, as jnp.sum(T_spin) (transport.py:181)
    for (int i = 0; rc >= 0 && i < m; ++i) T[i] = ((Tspin[4 * i] + Tspin[4 * i + 1]) + Tspin[4 * i + 2]) + Tspin[4 * i + 3];
    return rc;
}

int negf_dos(negf_ctx* c, int handle, int m, const double* E, double* dos_total, double* dos_site,
             int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (m > 0 && (!E || !dos_total)) return NEGF_EINVAL;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr))) return rc;
    rc = dense_batches(c, p, m, [&](int m0, int nb) {
        if (int e = run_assemble_inverse(c, p, m0, nb, c->d_E)) return e;
        { ProfScope ps(c, "trace"); launch_dos(c->stream, c->n, nb, c->G, c->d_scal + m0, dos_site ? c->d_site : nullptr); }
        return dos_site ? download(c, dos_site + (size_t)m0 * c->n, c->d_site, (size_t)nb * c->n) : NEGF_OK;
    });
    return rc ? rc : fetch_pageable(c, m, {{dos_total, c->d_scal, (size_t)m}}, info);
}

int negf_sigma_eval(negf_ctx* c, int handle, int contact, int m, const double* E, double* sigma_out,
                    int* iters, int* converged)
{
    SigmaProvider* p;
    int ct;
    int rc = open_call(c, handle, m, &p, contact, &ct);
    if (rc) return rc;
    if (m > 0 && (!E || !sigma_out)) return NEGF_EINVAL;
    const size_t n2 = (size_t)c->n * c->n;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr))) return rc;
    cplx* out = reinterpret_cast<cplx*>(sigma_out);
    rc = dense_batches(c, p, m, [&](int m0, int nb) {
        int e;
        switch (p->kind) {
        case SK_CONST: {
            const cplx* src = ct < 0 ? p->d_const_tot : p->d_const_c + n2 * ct;
            for (int b = 0; b < nb; ++b)
                if ((e = download(c, out + n2 * (m0 + b), src, n2))) return e;
            return NEGF_OK;
        }
        case SK_PRECOMPUTED: {
            if (ct < 0 || !p->d_pre_c) return download(c, out + n2 * m0, p->d_pre_tot + n2 * m0, n2 * nb);
            const int pn = std::max(p->pre_nc, 1);
            for (int b = 0; b < nb; ++b)
                if ((e = download(c, out + n2 * (m0 + b), p->d_pre_c + n2 * ((size_t)(m0 + b) * pn + ct), n2))) return e;
            return NEGF_OK;
        }
        case SK_CHAIN1D:
        case SK_BETHE: {
            if ((e = run_sigma_blocks(c, p, nb, c->d_E + m0, c->d_iters + (size_t)m0 * p->n_contacts,
                                      c->d_conv + (size_t)m0 * p->n_contacts, m0))) return e;
            launch_scatter_blocks(c->stream, c->n, nb, c->d_blk, p->blk_stride, p->n_contacts, p->d_nc,
                                  p->d_blk_off, p->d_inds_off, p->d_inds, ct, c->d_A);
            if (p->d_xi) {
                launch_zgemm(c->stream, c->n, c->n, c->n, nb, p->d_xi, c->n, 0, c->d_A, c->n, n2, 0, c->d_T2, c->n, n2);
                launch_zgemm(c->stream, c->n, c->n, c->n, nb, c->d_T2, c->n, n2, p->d_xi, c->n, 0, 0, c->d_A, c->n, n2);
            }
            return download(c, out + n2 * m0, c->d_A, n2 * nb);
        }
        default: return NEGF_EINVAL;
        }
    });
    return rc ? rc : fetch_iters(c, p, m, iters, converged);
}

int negf_bethe_raw(negf_ctx* c, const double* H, const double* Slist, const double* Vlist, double eta,
                   double conv, double mix, int max_iter, int force_iters, int which, int m,
                   const double* E, double* out, int* iters, int* converged)
{
    if (!c || !H || !Slist || !Vlist || m < 0 || (which != 1 && which != 2)) return NEGF_EINVAL;
    if (m > 0 && (!E || !out)) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    const int nd = which == 1 ? 12 : 9;
    double *dH = nullptr, *dS = nullptr, *dV = nullptr;
    cplx *dE = nullptr, *dout = nullptr;
    int *dit = nullptr, *dcv = nullptr;
    int rc = NEGF_OK;
    if ((rc = dev_alloc(&dH, 81)) || (rc = dev_alloc(&dS, 12 * 81)) || (rc = dev_alloc(&dV, 12 * 81)) ||
        (rc = dev_alloc(&dE, (size_t)m)) || (rc = dev_alloc(&dout, (size_t)m * nd * 81)) ||
        (rc = dev_alloc(&dit, (size_t)m)) || (rc = dev_alloc(&dcv, (size_t)m))) goto done;
    if ((rc = upload(c, dH, H, 81)) || (rc = upload(c, dS, Slist, 12 * 81)) || (rc = upload(c, dV, Vlist, 12 * 81)) ||
        (rc = upload(c, dE, reinterpret_cast<const cplx*>(E), (size_t)m))) goto done;
    {
        ProfScope ps(c, "bethe");
        launch_bethe_raw(c->stream, dH, dS, dV, eta, conv, mix, max_iter, force_iters, which, m, dE, dout, dit, dcv);
    }
    if ((rc = download(c, reinterpret_cast<cplx*>(out), dout, (size_t)m * nd * 81))) goto done;
    if (iters && (rc = download(c, iters, dit, (size_t)m))) goto done;
    if (converged && (rc = download(c, converged, dcv, (size_t)m))) goto done;
    if (hipGetLastError() != hipSuccess) rc = NEGF_EHIP;
done:
    dev_free(dH); dev_free(dS); dev_free(dV); dev_free(dE); dev_free(dout); dev_free(dit); dev_free(dcv);
    return rc;
}

// ---------------------------------------------------------------- eigenchannels and their scattering states
// T(E) = sum_n T_n(E), T_n the eigenvalues of t^H t, t = Gamma_R^{1/2} G_RL Gamma_L^{1/2}.  On a contact s with orbital
// list I_s (o the other one): Gamma_s = L L^H by pivoted Cholesky, and the T_n are the eigenvalues of H = L^H B L,
// B = G_so Gamma_o G_so^H, G_so = G[I_s, I_o].  Per energy: Z = L^H G_so (K_s x K_o), W = Z Gamma_o, H = W Z^H -- three
// small batched products -- and the Jacobi eigenproblem of H's leading rank x rank block.
//   negf_transmission_channels: s = the contact with the smaller list (L unless K_R < K_L), eigenvalues only.  The block
//     is gathered as G[I_L, I_R] either way: with s = R it enters the first product conjugate-transposed (the MIRROR form).
//   negf_channel_states: s = the SOURCE contact always (no division by sqrt(T_n): closed channels keep well-defined
//     states), in the mirror form (G[I_d, I_s] gathered); psi_n = G[:, I_s] L u_n with H u_n = T_n u_n.  The eigenvector
//     kernel starts its accumulator from L, so it leaves C = L U, stored as C^H; conj(Psi) = C^H G[:, I_s]^H is one
//     product, and the gauge pass conjugates it back while it fixes the phases.
namespace {

// providers whose Gamma_c is confined to a known orbital list
bool gamma_on_lists(const SigmaProvider* p)
{
    return (p->kind == SK_CONST && p->has_blocks) || ((p->kind == SK_CHAIN1D || p->kind == SK_BETHE) && !p->d_xi);
}

// The plan (who is s, who is o, which form) and, once chan_carve has run, the work area of the batch in c->d_chan:
// G_so | Z | W (K_s K_o each) | H (K_s^2) | mid | L^H | tail per energy -- L^H once for a CONST provider (Gamma does not
// depend on E: factored once per call) --, sized here, not carved out of the n x n workspace (contact lists may cover
// more than half of the orbitals).  mid and tail are the caller's (the states' C^H and eigenvector scratch).
struct ChanWork {
    int cs, co, Ks, Ko;
    bool mirror;                // G[I_o, I_s] is gathered and enters Z conjugate-transposed
    int s_slot;                 // the slot of run_gamma_small that takes Gamma_s; Gamma_o takes the other one
    bool constant;
    size_t kk, ks2, lstride;
    cplx *Gso, *Z, *W, *H, *mid, *Lh, *tail;
};

int chan_plan(negf_ctx* c, SigmaProvider* p, int contact_L, int contact_R, ChanWork* w)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (!p) return NEGF_EINVAL;
    if (!gamma_on_lists(p)) return NEGF_EINVAL;
    const int cL = norm_contact(p, contact_L), cR = norm_contact(p, contact_R);
    if (cL < 0 || cR < 0) return NEGF_EINVAL;                   // (the total self-energy is not a contact)
    w->mirror = p->nc[cR] < p->nc[cL];
    w->s_slot = w->mirror ? 1 : 0;                              // (Gamma_L goes to slot 0, Gamma_R to slot 1)
    w->cs = w->mirror ? cR : cL; w->co = w->mirror ? cL : cR;
    w->Ks = p->nc[w->cs]; w->Ko = p->nc[w->co];
    if (w->Ks > channels_kmax()) return NEGF_EINVAL;
    return NEGF_OK;
}

int state_plan(negf_ctx* c, SigmaProvider* p, int contact_src, int contact_dst, bool need_dst, ChanWork* w)
{
    if (!c || c->n <= 0) return NEGF_ESTATE;
    if (!p) return NEGF_EINVAL;
    if (!gamma_on_lists(p)) return NEGF_EINVAL;
    const int cs = norm_contact(p, contact_src), cd = need_dst ? norm_contact(p, contact_dst) : cs;
    if (cs < 0 || cd < 0) return NEGF_EINVAL;                   // (the total self-energy is not a contact)
    w->cs = cs; w->co = cd; w->Ks = p->nc[cs]; w->Ko = p->nc[cd];
    w->mirror = true; w->s_slot = 0;
    if (w->Ks < 1 || w->Ko < 1 || w->Ks > channels_kmax()) return NEGF_EINVAL;   // (K_d is not limited)
    return NEGF_OK;
}

int chan_carve(negf_ctx* c, SigmaProvider* p, ChanWork* w, int batch, size_t mid_per, size_t tail_per)
{
    w->constant = p->kind == SK_CONST;
    w->kk = (size_t)w->Ks * w->Ko; w->ks2 = (size_t)w->Ks * w->Ks; w->lstride = w->constant ? 0 : w->ks2;
    const size_t nl = w->constant ? 1 : (size_t)batch;          // factors L^H and their pivoted Cholesky ranks
    int rc;
    if ((rc = ensure_cap(c, c->d_chan, (3 * w->kk + w->ks2 + mid_per + tail_per) * batch + w->ks2 * nl)) ||
        (rc = ensure_cap(c, c->d_chan_rank, nl))) return rc;
    w->Gso = c->d_chan;
    w->Z = w->Gso + w->kk * batch;
    w->W = w->Z + w->kk * batch;
    w->H = w->W + w->kk * batch;
    w->mid = w->H + w->ks2 * batch;
    w->Lh = w->mid + mid_per * batch;
    w->tail = w->Lh + w->ks2 * nl;
    return NEGF_OK;
}

// G of the batch [m0, m0 + nb), the two Gammas, L^H (once per call for a CONST provider), and H; *gs: Gamma_s and I_s
int chan_build_H(negf_ctx* c, SigmaProvider* p, const ChanWork& w, int m0, int nb, const cplx* E, GammaSmall* gs)
{
    int rc;
    const int n = c->n, Ks = w.Ks, Ko = w.Ko;
    const size_t n2 = (size_t)n * n, kk = w.kk;
    if ((rc = run_assemble_inverse(c, p, m0, nb, E))) return rc;
    GammaSmall g[2];
    {
        ProfScope ps(c, "gamma");
        if ((rc = run_gamma_small(c, p, w.s_slot ? w.co : w.cs, nb, 0, &g[0]))) return rc;
        if ((rc = run_gamma_small(c, p, w.s_slot ? w.cs : w.co, nb, 1, &g[1]))) return rc;
    }
    const GammaSmall& go = g[1 - w.s_slot];
    *gs = g[w.s_slot];
    if (!w.constant || m0 == 0) {
        ProfScope ps(c, "eig");
        if (!launch_pivoted_cholesky(c->stream, Ks, w.constant ? 1 : nb, gs->mat, gs->stride, w.Lh, w.ks2, c->d_chan_rank))
            return NEGF_EINVAL;
    }
    ProfScope ps(c, "zgemm");
    const GammaSmall& rows = w.mirror ? go : *gs;
    const GammaSmall& cols = w.mirror ? *gs : go;
    launch_gather_block(c->stream, n, rows.K, cols.K, nb, c->G, n2, rows.idx, cols.idx, w.Gso, kk);
    // Z = L^H G_so: the block as it is (K_s x K_o), or gathered K_o x K_s and conjugate-transposed on the way (stored
    // N x K, opB = 1) in the mirror form; W = Z Gamma_o; H = W Z^H
    launch_zgemm(c->stream, Ks, Ko, Ks, nb, w.Lh, Ks, w.lstride, w.Gso, w.mirror ? Ks : Ko, kk, w.mirror ? 1 : 0, w.Z, Ko, kk);
    launch_zgemm(c->stream, Ks, Ko, Ko, nb, w.Z, Ko, kk, go.mat, Ko, go.stride, 0, w.W, Ko, kk);
    launch_zgemm(c->stream, Ks, Ks, Ko, nb, w.W, Ko, kk, w.Z, Ko, kk, 1, w.H, Ks, w.ks2);
    return NEGF_OK;
}

// negf_eigvalsh_batched (V null) and negf_eigh_batched: m Hermitian K x K matrices up, w and V down
int eigh_host(negf_ctx* c, int K, int m, const double* A, double* w, double* V, int* info)
{
    if (!c) return NEGF_EINVAL;
    if (K < 1 || K > channels_kmax() || m < 0 || (m > 0 && (!A || !w))) return NEGF_EINVAL;
    if (m == 0) return NEGF_OK;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    const size_t k2 = (size_t)K * K, xg_per = V ? eigh_scratch_elems(K) : 0;
    cplx *dA = nullptr, *dV = nullptr, *dx = nullptr; double* dw = nullptr; int* di = nullptr;
    std::vector<int> hi((size_t)m);
    // (one way out: whatever fails, everything allocated so far is freed below)
    int rc = dev_alloc(&dA, k2 * m);
    if (!rc && V) rc = dev_alloc(&dV, k2 * m);
    if (!rc) rc = dev_alloc(&dw, (size_t)K * m);
    if (!rc) rc = dev_alloc(&di, (size_t)m);
    if (!rc && xg_per) rc = dev_alloc(&dx, xg_per * m);
    if (!rc) rc = upload(c, dA, reinterpret_cast<const cplx*>(A), k2 * m);
    if (!rc) {
        ProfScope ps(c, "eig");
        JacVec v{};
        v.xg = dx;
        v.out = dV; v.out_stride = k2; v.out_ri = K; v.out_cj = 1; v.ncol = K;      // eigenvector j in column j
        const bool ok = V ? launch_eigh_batched(c->stream, K, m, dA, K, k2, nullptr, 0, dw, K, K, false, di, false, 1, v)
                          : launch_eigvalsh_batched(c->stream, K, m, dA, K, k2, nullptr, 0, dw, K, K, false, di, false, 1);
        if (!ok) rc = NEGF_EINVAL;
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = NEGF_EHIP;
    if (!rc) rc = download(c, w, dw, (size_t)K * m);
    if (!rc && V) rc = download(c, reinterpret_cast<cplx*>(V), dV, k2 * m);
    if (!rc) rc = download(c, hi.data(), di, (size_t)m);
    dev_free(dA); dev_free(dV); dev_free(dw); dev_free(di); dev_free(dx);
    if (rc) return rc;
    for (int i = 0; i < m; ++i) {
        if (info) info[i] = hi[i];
        if (hi[i] != 0) rc = NEGF_ESINGULAR;
    }
    return rc;
}

}  // namespace

int negf_channel_count(negf_ctx* c, int handle, int contact_L, int contact_R, int* nchan)
{
    if (!nchan) return NEGF_EINVAL;
    ChanWork w;
    const int rc = chan_plan(c, get_provider(c, handle), contact_L, contact_R, &w);
    if (rc) return rc;
    *nchan = w.Ks;
    return NEGF_OK;
}

int negf_transmission_channels_dev(negf_ctx* c, int handle, int contact_L, int contact_R, int m, const double* E_dev,
                                   int nchan, double* T_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    ChanWork w;
    if ((rc = chan_plan(c, p, contact_L, contact_R, &w))) return rc;
    if (nchan < 1 || !T_dev || (m > 0 && !E_dev)) return NEGF_EINVAL;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    return dense_batches(c, p, m, [&](int batch) { return chan_carve(c, p, &w, batch, 0, 0); }, [&](int m0, int nb) {
        GammaSmall gs;
        if (int e = chan_build_H(c, p, w, m0, nb, E, &gs)) return e;
        ProfScope ps(c, "eig");
        // (the rank of a CONST factor serves every energy: rank stride 0.  All nchan columns are written: values,
        //  zeros beyond the rank or K_s, or a whole NaN row for a singular energy)
        return launch_eigvalsh_batched(c->stream, w.Ks, nb, w.H, w.Ks, w.ks2, c->d_chan_rank, w.constant ? 0 : 1,
                                       T_dev + (size_t)m0 * nchan, nchan, nchan, true, c->d_info + m0, true, -1) ? NEGF_OK : NEGF_EINVAL;
    });
}

int negf_transmission_channels(negf_ctx* c, int handle, int contact_L, int contact_R, int m, const double* E,
                               int nchan, double* T_chan, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (nchan < 1 || (m > 0 && (!E || !T_chan))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * nchan;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_chan_T, cnt))) return rc;
    if ((rc = negf_transmission_channels_dev(c, handle, contact_L, contact_R, m, dev_E(c), nchan, c->d_chan_T))) return rc;
    return fetch_pageable(c, m, {{T_chan, c->d_chan_T.p, cnt}}, info);
}

int negf_eigvalsh_batched(negf_ctx* c, int K, int m, const double* A, double* w, int* info)
{
    return eigh_host(c, K, m, A, w, nullptr, info);
}

int negf_channel_states_count(negf_ctx* c, int handle, int contact_src, int* count)
{
    if (!count) return NEGF_EINVAL;
    ChanWork w;
    const int rc = state_plan(c, get_provider(c, handle), contact_src, 0, false, &w);
    if (rc) return rc;
    *count = w.Ks;
    return NEGF_OK;
}

int negf_channel_states_dev(negf_ctx* c, int handle, int contact_src, int contact_dst, int m, const double* E_dev,
                            int nchan, double* T_dev, double* psi_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    ChanWork w;
    if ((rc = state_plan(c, p, contact_src, contact_dst, true, &w))) return rc;
    if (nchan < 1 || !T_dev || !psi_dev || (m > 0 && !E_dev)) return NEGF_EINVAL;
    const int n = c->n, Ks = w.Ks;
    const size_t n2 = (size_t)n * n;
    const int nce = std::min(nchan, Ks);                     // channels computed; the columns beyond are zeros
    // behind H: C^H (K_s^2 per energy); behind L^H: the eigenvector kernel's scratch.  G[:, I_s] and conj(Psi) (n K_s,
    // nce n <= n^2) go to the free n x n work areas W2 and W1
    const size_t xg_per = eigh_scratch_elems(Ks);
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    cplx* psi = reinterpret_cast<cplx*>(psi_dev);
    return dense_batches(c, p, m, [&](int batch) { return chan_carve(c, p, &w, batch, (size_t)Ks * Ks, xg_per); }, [&](int m0, int nb) {
        GammaSmall gs;
        if (int e = chan_build_H(c, p, w, m0, nb, E, &gs)) return e;
        cplx* Ch = w.mid;
        {
            ProfScope ps(c, "eig");
            // X0 = L, read out of L^H; the sorted columns of C = L U leave as the rows of C^H (nce x K_s)
            JacVec v{};
            v.x0 = w.Lh; v.x0_stride = w.lstride; v.x0_ri = 1; v.x0_cj = Ks; v.x0_conj = 1;
            v.xg = xg_per ? w.tail : nullptr;
            v.out = Ch; v.out_stride = w.ks2; v.out_ri = 1; v.out_cj = Ks; v.out_conj = 1; v.ncol = nce;
            if (!launch_eigh_batched(c->stream, Ks, nb, w.H, Ks, w.ks2, c->d_chan_rank, w.constant ? 0 : 1, T_dev + (size_t)m0 * nchan,
                                     nchan, nchan, true, c->d_info + m0, true, -1, v)) return NEGF_EINVAL;
        }
        ProfScope ps(c, "zgemm");
        launch_gather_block(c->stream, n, n, Ks, nb, c->G, n2, nullptr, gs.idx, c->W2, n2);
        // conj(Psi) = C^H G[:, I_s]^H (nce x n; G[:, I_s] stored n x K_s: opB = 1)
        launch_zgemm(c->stream, nce, n, Ks, nb, Ch, Ks, w.ks2, c->W2, Ks, n2, 1, c->W1, n, n2);
        launch_channel_gauge(c->stream, n, nce, nchan, nb, c->W1, n2, c->d_chan_rank, w.constant ? 0 : 1, c->d_info + m0,
                             psi + (size_t)m0 * nchan * n);
        return NEGF_OK;
    });
}

int negf_channel_states(negf_ctx* c, int handle, int contact_src, int contact_dst, int m, const double* E, int nchan,
                        double* T_chan, double* psi, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (nchan < 1 || (m > 0 && (!E || !T_chan || !psi))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * nchan, pcnt = cnt * c->n;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_chan_T, std::max<size_t>(cnt, 1))) ||
        (rc = ensure_cap(c, c->d_chan_psi, std::max<size_t>(pcnt, 1)))) return rc;
    if ((rc = negf_channel_states_dev(c, handle, contact_src, contact_dst, m, dev_E(c), nchan,
                                      c->d_chan_T, reinterpret_cast<double*>(c->d_chan_psi.p)))) return rc;
    return fetch_pageable(c, m, {{T_chan, c->d_chan_T.p, cnt}, {reinterpret_cast<cplx*>(psi), c->d_chan_psi.p, pcnt}}, info);
}

int negf_eigh_batched(negf_ctx* c, int K, int m, const double* A, double* w, double* V, int* info)
{
    if (m > 0 && !V) return NEGF_EINVAL;
    return eigh_host(c, K, m, A, w, V, info);
}

// ------------------------------------------------------- the blocked inverse's launch rule (diagnostic)
int negf_inverse_plan(int n, int nb, int algo, int defer, int* path, int* nbi, int* rpt, int* nblk, int* groups,
                      int* group_tab, int* gather, int* deferred)
{
    if (n < 1 || nb < 1 || algo < 0 || algo > 4) return NEGF_EINVAL;
    GjPlan pl;
    if (algo != 1) {                     // (1: the unblocked kernel, path 0)
        const int rc = gj_plan(n, nb, algo == 3 ? 1 : algo == 4 ? 2 : 0, defer != 0, gj_params(), &pl);
        if (rc) return rc;
    }
    if (path) *path = pl.path;
    if (nbi) *nbi = pl.nbi;
    if (rpt) *rpt = pl.rpt;
    if (nblk) *nblk = pl.nblk;
    if (groups) *groups = pl.groups;
    if (gather) *gather = pl.gather;
    if (deferred) *deferred = pl.deferred;
    if (group_tab)
        for (int g = 0; g < 4; ++g) {
            const GjGroup& gp = pl.g[g];
            const int row[7] = {gp.first, gp.count, gp.wk, gp.pairs, gp.upd_full, gp.upd_single, (int)gp.mask};
            for (int k = 0; k < 7; ++k) group_tab[g * 7 + k] = g < pl.groups ? row[k] : 0;
        }
    return NEGF_OK;
}

int negf_inverse_last(negf_ctx* c, int* path, int* groups, int* masks)
{
    if (!c) return NEGF_EINVAL;
    if (path) *path = c->gj_last.path;
    if (groups) *groups = c->gj_last.groups;
    if (masks) for (int g = 0; g < 4; ++g) masks[g] = (int)c->gj_last.mask[g];
    return NEGF_OK;
}

// ------------------------------------------------------- the product kernels, called directly (diagnostic)
int negf_zgemm_plan(int M, int N, int K, int opB, int nb, int kernel, int* kernel_used, int* opB_eff, int* blocks,
                    int* grid, int* decode, int decode_cap)
{
    return zgemm_plan(M, N, K, opB, nb, kernel, kernel_used, opB_eff, blocks, grid, decode, decode_cap);
}

int negf_zgemm_batched(negf_ctx* c, int M, int N, int K, int nb, const double* A, int lda, long long strideA,
                       const double* B, int ldb, long long strideB, int opB, double* C, int ldc, long long strideC,
                       int kernel)
{
    if (!c || M < 1 || N < 1 || K < 0 || nb < 1 || opB < 0 || opB > 7 || kernel < ZGEMM_AUTO || kernel > ZGEMM_VALU) return NEGF_EINVAL;
    if (!A || !B || !C) return NEGF_EINVAL;
    const bool bh = (opB & 1) != 0, ct = (opB & 4) != 0;
    const long long b_rows = bh ? N : K, b_cols = bh ? K : N, c_rows = ct ? N : M, c_cols = ct ? M : N;
    if (lda < std::max(K, 1) || ldb < std::max<long long>(b_cols, 1) || ldc < c_cols) return NEGF_EINVAL;
    const long long ea = (long long)M * lda, eb = b_rows * ldb, ec = c_rows * ldc;
    if ((strideA != 0 && strideA < ea) || (strideB != 0 && strideB < eb) || strideC < ec) return NEGF_EINVAL;
    const long long na = strideA ? strideA * nb : ea, nbb = strideB ? strideB * nb : eb, nc = strideC * nb;
    if (std::max(na, std::max(nbb, nc)) > (1LL << 31)) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    cplx *dA = nullptr, *dB = nullptr, *dC = nullptr;
    int rc;
    if ((rc = dev_alloc(&dA, (size_t)na)) || (rc = dev_alloc(&dB, (size_t)nbb)) || (rc = dev_alloc(&dC, (size_t)nc))) {
        dev_free(dA); dev_free(dB); return rc;
    }
    if (!(rc = upload(c, dA, reinterpret_cast<const cplx*>(A), (size_t)na)) &&
        !(rc = upload(c, dB, reinterpret_cast<const cplx*>(B), (size_t)nbb)) &&
        !(rc = upload(c, dC, reinterpret_cast<const cplx*>(C), (size_t)nc))) {
        ProfScope ps(c, "zgemm");
        launch_zgemm_as(c->stream, kernel, true, M, N, K, nb, dA, lda, (size_t)strideA, dB, ldb, (size_t)strideB, opB,
                        dC, ldc, (size_t)strideC);
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = NEGF_EHIP;
    if (!rc) rc = download(c, reinterpret_cast<cplx*>(C), dC, (size_t)nc);
    dev_free(dA); dev_free(dB); dev_free(dC);
    return rc;
}

// ------------------------------------------------------- local (bond) transmission
// flow[i][j](E) = 2 Im[(E S - F)_ij A_c,ji],  A_c = G Gamma_c G^H: the GrLessInt sequence up to A_c (run_gless_products),
// then one pass of k_bond.hip over A_c where GrLessInt runs launch_accumulate.  The reference has no such function.
namespace {

// providers served: all that negf_gless_int serves, except coupling matrices handed in by the caller (they need not
// be Hermitian, and the kernels read A_ji as conj(A_ij))
int bond_open(negf_ctx* c, int handle, int m, int ind, SigmaProvider** p, int* contact)
{
    int rc = open_call(c, handle, m, p, ind, contact);
    if (rc) return rc;
    if ((*p)->kind == SK_PRECOMPUTED && (*p)->pre_is_gamma) return NEGF_EINVAL;
    return c->n > bond_max_n() ? NEGF_EINVAL : NEGF_OK;
}

// The orbital -> group map sorted once per call: perm = the orbitals by group, ascending inside a group; goff = the
// groups' offsets in perm (both on the device).  Both null: every orbital is its own group, in order (the elementwise
// kernel serves it).
struct BondMap { const int *perm = nullptr, *goff = nullptr; };
int bond_stage_groups(negf_ctx* c, int n_groups, const int* group_of, BondMap* bm)
{
    const int n = c->n;
    bool identity = true;
    if (!group_of) return n_groups == n ? NEGF_OK : NEGF_EINVAL;
    if (n_groups < 1 || n_groups > n) return NEGF_EINVAL;
    for (int i = 0; i < n; ++i) {
        if (group_of[i] < 0 || group_of[i] >= n_groups) return NEGF_EINVAL;
        if (group_of[i] != i) identity = false;
    }
    if (identity && n_groups == n) return NEGF_OK;
    std::vector<int> map((size_t)n + n_groups + 1, 0);
    int* perm = map.data();
    int* goff = map.data() + n;
    for (int i = 0; i < n; ++i) ++goff[group_of[i] + 1];
    for (int g = 0; g < n_groups; ++g) goff[g + 1] += goff[g];
    std::vector<int> next(goff, goff + n_groups);
    for (int i = 0; i < n; ++i) perm[next[group_of[i]]++] = i;
    int rc = ensure_cap(c, c->d_bond_map, map.size());
    if (rc) return rc;
    bm->perm = c->d_bond_map; bm->goff = c->d_bond_map + n;
    return upload(c, c->d_bond_map.p, map.data(), map.size());
}

}  // namespace

int negf_local_transmission_dev(negf_ctx* c, int handle, int ind, int m, const double* E_dev, int n_groups,
                                const int* group_of, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = bond_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if (m > 0 && (!E_dev || !out_dev)) return NEGF_EINVAL;
    BondMap bm;
    if ((rc = bond_stage_groups(c, n_groups, group_of, &bm))) return rc;
    const int n = c->n;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    const size_t tab = (size_t)n_groups * n_groups;
    return dense_batches(c, p, m, [&](int m0, int nb) {
        if (int e = run_gless_products(c, p, contact, m0, nb, E)) return e;
        ProfScope ps(c, "bond");
        return launch_bond_tables(c->stream, n, nb, E + m0, c->d_S, c->d_F, c->W1, c->d_info + m0, n_groups, bm.perm, bm.goff,
                                  out_dev + tab * m0) ? NEGF_OK : NEGF_EINVAL;
    });
}

int negf_local_transmission(negf_ctx* c, int handle, int ind, int m, const double* E, int n_groups, const int* group_of,
                            double* out, int* info)
{
    SigmaProvider* p;
    int contact;
    int rc = bond_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if (n_groups < 1 || (m > 0 && (!E || !out))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * n_groups * n_groups;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_local_transmission_dev(c, handle, ind, m, dev_E(c), n_groups, group_of, c->d_bond_T))) return rc;
    return fetch_pageable(c, m, {{out, c->d_bond_T.p, cnt}}, info);
}

int negf_bond_int_dev(negf_ctx* c, int handle, int ind, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = bond_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    const size_t n2 = (size_t)c->n * c->n;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    auto setup = [&](int) {
        if (int e = ensure_cap(c, c->d_bond_carry, n2)) return e;
        return clear_first(c, out_dev, n2 * sizeof(double))(0);
    };
    return dense_batches(c, p, m, setup, [&](int m0, int nb) {
        if (int e = run_gless_products(c, p, contact, m0, nb, E)) return e;
        ProfScope ps(c, "bond");
        // (the chunk records go where the products' temporaries were: (nb / 32 + 2) n^2 doubles of W2's 2 nb n^2)
        launch_bond_int(c->stream, (int)n2, m, m0, nb, E + m0, w_dev + m0, c->d_S, c->d_F, c->W1, c->d_bond_carry,
                        reinterpret_cast<double*>(c->W2), out_dev);
        return NEGF_OK;
    });
}

int negf_bond_int(negf_ctx* c, int handle, int ind, int m, const double* E, const double* w, double* out, int* info)
{
    SigmaProvider* p;
    int contact;
    int rc = bond_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if (!out || (m > 0 && (!E || !w))) return NEGF_EINVAL;
    const size_t ob = (size_t)c->n * c->n * sizeof(double);
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = stage_real_weights(c, m, w, ob))) return rc;
    double* dout = dev_acc(c);          // n^2 doubles of its n^2 complex values
    if ((rc = negf_bond_int_dev(c, handle, ind, m, dev_E(c), dev_w(c), dout))) return rc;
    return fetch_result_and_info(c, m, dout, ob, out, info);
}

// ------------------------------------------------------- populations and projected DOS
// pop[i][j] = -(1/pi) Im[G_ij conj(X_ij)] (retarded) or (1/2 pi) Re[A_c,ij conj(X_ij)] (contact c), X = S or F: negf_dos's
// sequence up to G, or the GrLessInt sequence up to A_c (run_gless_products), then ONE pass of k_population.hip.  The
// reference has no such function.
namespace {

// ind = NEGF_IND_RETARDED: every provider negf_dos serves; otherwise what the local transmission serves (bond_open)
int pop_open(negf_ctx* c, int handle, int m, int ind, SigmaProvider** p, int* contact)
{
    if (ind != NEGF_IND_RETARDED) return bond_open(c, handle, m, ind, p, contact);
    *contact = -1;
    int rc = open_call(c, handle, m, p);
    if (rc) return rc;
    return c->n > bond_max_n() ? NEGF_EINVAL : NEGF_OK;
}

// G (retarded) or A_c (contact) of the batch [m0, m0 + nb); *free_area: a work area of nb n^2 values the result does not use
int pop_matrix(negf_ctx* c, SigmaProvider* p, int ind, int contact, int m0, int nb, const cplx* E, const cplx** M,
               cplx** free_area)
{
    int rc;
    if (ind == NEGF_IND_RETARDED) {
        if ((rc = run_assemble_inverse(c, p, m0, nb, E))) return rc;
        *M = c->G; *free_area = c->W1;
        return NEGF_OK;
    }
    if ((rc = run_gless_products(c, p, contact, m0, nb, E))) return rc;
    *M = c->W1; *free_area = c->W2;
    return NEGF_OK;
}

}  // namespace

int negf_population_dev(negf_ctx* c, int handle, int ind, int op, int rows_only, int m, const double* E_dev, int n_groups,
                        const int* group_of, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = pop_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if ((op != 0 && op != 1) || (rows_only != 0 && rows_only != 1)) return NEGF_EINVAL;
    if (m > 0 && (!E_dev || !out_dev)) return NEGF_EINVAL;
    BondMap bm;
    if ((rc = bond_stage_groups(c, n_groups, group_of, &bm))) return rc;
    const int n = c->n;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    const cplx* X = op == 0 ? c->d_S : c->d_F;
    const size_t per = rows_only ? (size_t)n_groups : (size_t)n_groups * n_groups;
    return dense_batches(c, p, m, [&](int m0, int nb) {
        const cplx* M;
        cplx* unused;
        if (int e = pop_matrix(c, p, ind, contact, m0, nb, E, &M, &unused)) return e;
        ProfScope ps(c, "pop");
        return launch_population(c->stream, n, nb, ind == NEGF_IND_RETARDED, X, M, c->d_info + m0, rows_only, n_groups, bm.perm,
                                 bm.goff, out_dev + per * m0) ? NEGF_OK : NEGF_EINVAL;
    });
}

int negf_population(negf_ctx* c, int handle, int ind, int op, int rows_only, int m, const double* E, int n_groups,
                    const int* group_of, double* out, int* info)
{
    SigmaProvider* p;
    int contact;
    int rc = pop_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    if (n_groups < 1 || n_groups > c->n || (rows_only != 0 && rows_only != 1) || (m > 0 && (!E || !out))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * n_groups * (rows_only ? 1 : n_groups);
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_population_dev(c, handle, ind, op, rows_only, m, dev_E(c), n_groups, group_of, c->d_bond_T))) return rc;
    return fetch_pageable(c, m, {{out, c->d_bond_T.p, cnt}}, info);
}

int negf_projected_dos_dev(negf_ctx* c, int handle, int ind, int m, const double* E_dev, int k, const double* W_dev,
                           double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = pop_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    const int n = c->n;
    if (k < 1 || k > n || !W_dev || (m > 0 && (!E_dev || !out_dev))) return NEGF_EINVAL;
    if (m == 0) { c->last_m = 0; return NEGF_OK; }
    const size_t nk = (size_t)n * k, n2 = (size_t)n * n;
    if ((rc = ensure_cap(c, c->d_pop_Wt, nk))) return rc;
    cplx* Wt = c->d_pop_Wt;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    auto setup = [&](int) {
        ProfScope ps(c, "pop");
        launch_pop_transpose_w(c->stream, n, k, reinterpret_cast<const cplx*>(W_dev), Wt);
        return NEGF_OK;
    };
    return dense_batches(c, p, m, setup, [&](int m0, int nb) {
        const cplx* M;
        cplx* Y;
        if (int e = pop_matrix(c, p, ind, contact, m0, nb, E, &M, &Y)) return e;
        // Y_b = M_b Wt (n x k): Wt shared by the batch
        { ProfScope ps(c, "zgemm"); launch_zgemm(c->stream, n, k, n, nb, M, n, n2, Wt, k, 0, 0, Y, k, nk); }
        ProfScope ps(c, "pop");
        launch_pop_coldot(c->stream, n, k, nb, ind == NEGF_IND_RETARDED, Wt, Y, nk, c->d_info + m0, out_dev + (size_t)k * m0);
        return NEGF_OK;
    });
}

int negf_projected_dos(negf_ctx* c, int handle, int ind, int m, const double* E, int k, const double* W, double* out,
                       int* info)
{
    SigmaProvider* p;
    int contact;
    int rc = pop_open(c, handle, m, ind, &p, &contact);
    if (rc) return rc;
    const int n = c->n;
    if (k < 1 || k > n || !W || (m > 0 && (!E || !out))) return NEGF_EINVAL;
    const size_t nk = (size_t)n * k, cnt = (size_t)m * k;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_pop_W, nk)) ||
        (rc = upload(c, c->d_pop_W.p, reinterpret_cast<const cplx*>(W), nk)) || (rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_projected_dos_dev(c, handle, ind, m, dev_E(c), k,
                                     reinterpret_cast<const double*>(c->d_pop_W.p), c->d_bond_T))) return rc;
    return fetch_pageable(c, m, {{out, c->d_bond_T.p, cnt}}, info);
}

// ------------------------------------------------- multi-terminal transmission matrix
// T[a][b](E) = Re Tr[Gamma_a G Gamma_b G^H] between all C terminals -- the provider's contacts followed by the call's
// probes -- from one inverse per energy (k_tmatrix.hip).  The probes' Sigma blocks enter A = E S - F - Sigma through an
// n x n copy of F (of F + Sigma_tot for a CONST provider) that carries them and stands in for the original while the
// call assembles; no existing kernel knows about probes.  The reference has no such function.
namespace {

// the copy of F / hbase with the probes added stands in for the original until the guard goes out of scope
struct TmatSwap {
    cplx** slot = nullptr; cplx* keep = nullptr;
    void set(cplx** s, cplx* with) { slot = s; keep = *s; *s = with; }
    ~TmatSwap() { if (slot) *slot = keep; }
};

struct TmatPlan {
    int C = 0, nc = 0, n_probes = 0;
    const cplx* psig = nullptr;                            // the caller's probe blocks (host)
    std::vector<int> K, ioff, goff, gstride, soff, order, idx;
    std::vector<int> pairs[3];                             // by tmat_pair_class
    int max_elems[3] = {0, 0, 0};
    size_t psum = 0, csum = 0, big_kk = 0;                 // sum K_p^2, sum K_c^2, largest K_a K_b of class 0
    bool per_energy = false;                               // the contacts' Gamma blocks depend on E (block providers)
};

// The content order of two probes a and b (terminal numbers): size, then orbital list (idx at ioff), then the block's
// values (sigma at soff) compared as numbers.  The dense and the layered path add their probes to H in this one order,
// which is what keeps the two bit for bit alike whatever order the caller names the probes in.
bool tmat_probe_before(const std::vector<int>& K, const std::vector<int>& idx, const std::vector<int>& ioff, const cplx* sigma,
                       const std::vector<int>& soff, int a, int b)
{
    const int ka = K[a], kb = K[b];
    if (ka != kb) return ka < kb;
    const int* ia = idx.data() + ioff[a];
    const int* ib = idx.data() + ioff[b];
    for (int i = 0; i < ka; ++i) if (ia[i] != ib[i]) return ia[i] < ib[i];
    const double* sg = reinterpret_cast<const double*>(sigma);
    const double* xa = sg + 2 * (size_t)soff[a];
    const double* xb = sg + 2 * (size_t)soff[b];
    for (int i = 0; i < 2 * ka * ka; ++i) if (xa[i] != xb[i]) return xa[i] < xb[i];
    return false;
}

// providers whose Gamma_c is confined to a known orbital list, as for the eigenchannels; the probe lists are checked
int tmat_plan(negf_ctx* c, SigmaProvider* p, int n_probes, const int* probe_nk, const int* probe_inds,
              const cplx* probe_sigma, TmatPlan* pl)
{
    pl->n_probes = n_probes; pl->psig = probe_sigma;
    if (!gamma_on_lists(p) || !probes_count_ok(p, n_probes)) return NEGF_EINVAL;
    if (n_probes > 0 && (!probe_nk || !probe_inds || !probe_sigma)) return NEGF_EINVAL;
    const int n = c->n, nc = p->n_contacts;
    const int C = nc + n_probes;
    pl->C = C; pl->nc = nc; pl->per_energy = p->kind != SK_CONST;
    pl->K.resize(C); pl->ioff.resize(C); pl->goff.resize(C); pl->gstride.resize(C); pl->soff.resize(C);
    std::vector<size_t> sig_at(C, 0);
    size_t psum = 0, isum = 0;
    std::vector<char> seen(n);
    for (int q = 0; q < n_probes; ++q) {
        const int k = probe_nk[q];
        if (k < 1 || k > n) return NEGF_EINVAL;
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < k; ++i) {
            const int v = probe_inds[isum + i];
            if (v < 0 || v >= n || seen[v]) return NEGF_EINVAL;
            seen[v] = 1;
        }
        isum += k; psum += (size_t)k * k;
        if (psum > ((size_t)1 << 30)) return NEGF_EINVAL;
    }
    size_t csum = 0;
    for (int k : p->nc) csum += (size_t)k * k;
    if (csum > ((size_t)1 << 30)) return NEGF_EINVAL;
    pl->psum = psum; pl->csum = csum;
    pl->idx = p->h_inds;
    pl->idx.insert(pl->idx.end(), probe_inds, probe_inds + isum);
    for (int t = 0; t < nc; ++t) {
        pl->K[t] = p->nc[t]; pl->ioff[t] = p->inds_off[t]; pl->soff[t] = p->blk_off[t];
        pl->goff[t] = (int)psum + p->blk_off[t]; pl->gstride[t] = pl->per_energy ? (int)csum : 0;
    }
    int io = (int)p->h_inds.size(), so = 0;
    for (int q = 0; q < n_probes; ++q) {
        const int t = nc + q, k = probe_nk[q];
        pl->K[t] = k; pl->ioff[t] = io; pl->soff[t] = so; pl->goff[t] = so; pl->gstride[t] = 0;
        io += k; so += k * k;
    }
    // the order in which the probes are added to H: by content (orbital list, then the block's values compared as
    // numbers, which a scaling by a power of two keeps), so that it does not follow the caller's order
    pl->order.resize(n_probes);
    for (int q = 0; q < n_probes; ++q) pl->order[q] = nc + q;
    std::stable_sort(pl->order.begin(), pl->order.end(),
                     [&](int a, int b) { return tmat_probe_before(pl->K, pl->idx, pl->ioff, probe_sigma, pl->soff, a, b); });
    for (int a = 0; a < C; ++a)
        for (int b = 0; b < C; ++b) {
            const int cls = tmat_pair_class(pl->K[a], pl->K[b]);
            const int ne = pl->K[a] * pl->K[b];
            pl->pairs[cls].push_back(a * C + b);
            pl->max_elems[cls] = std::max(pl->max_elems[cls], ne);
            if (cls == 0) pl->big_kk = std::max(pl->big_kk, (size_t)pl->K[a] * pl->K[b]);
        }
    return NEGF_OK;
}

// What negf_transmission_matrix and the floating-probe calls share behind tmat_plan: the device tables, the probes added
// to the copy of F that stands in for the original while the call runs (swap), the Gamma blocks that do not depend on E.
// The set-up of their dense_batches: the workspace stands, so c->batch is the batch the areas are sized for.
struct TmatRun {
    TmatPlan pl;
    size_t pair_at[3] = {0, 0, 0};
    const int *dK = nullptr, *d_ioff = nullptr, *d_goff = nullptr, *d_gstride = nullptr, *d_soff = nullptr;
    const int *d_order = nullptr, *d_idx = nullptr;
    cplx* gam = nullptr;
    TmatSwap swap;
};

int tmat_setup(negf_ctx* c, SigmaProvider* p, TmatRun* r)
{
    int rc;
    const TmatPlan& pl = r->pl;
    const int n = c->n, C = pl.C, nc = pl.nc, n_probes = pl.n_probes;
    const size_t n2 = (size_t)n * n, C2 = (size_t)C * C;
    const int batch = c->batch;
    // the tables: K | ioff | goff | gstride | soff | probe order | orbital lists | the pair lists of the three classes
    std::vector<int> tab;
    tab.reserve((size_t)5 * C + n_probes + pl.idx.size() + C2);
    for (const std::vector<int>* v : {&pl.K, &pl.ioff, &pl.goff, &pl.gstride, &pl.soff, &pl.order, &pl.idx})
        tab.insert(tab.end(), v->begin(), v->end());
    for (int k = 0; k < 3; ++k) { r->pair_at[k] = tab.size(); tab.insert(tab.end(), pl.pairs[k].begin(), pl.pairs[k].end()); }
    if ((rc = ensure_cap(c, c->d_tmat_tab, tab.size())) || (rc = upload(c, c->d_tmat_tab.p, tab.data(), tab.size()))) return rc;
    const int* dK = c->d_tmat_tab;
    r->dK = dK; r->d_ioff = dK + C; r->d_goff = dK + 2 * C; r->d_gstride = dK + 3 * C; r->d_soff = dK + 4 * C;
    r->d_order = dK + 5 * C;
    r->d_idx = r->d_order + n_probes;
    if ((rc = ensure_cap(c, c->d_tmat_gam, pl.psum + pl.csum * (pl.per_energy ? batch : 1)))) return rc;
    if ((rc = ensure_cap(c, c->d_tmat_work, pl.big_kk * batch))) return rc;
    r->gam = c->d_tmat_gam;
    ProfScope ps(c, "tmat");
    if (n_probes > 0) {
        if ((rc = ensure_cap(c, c->d_tmat_sig, pl.psum)) || (rc = upload(c, c->d_tmat_sig.p, pl.psig, pl.psum))) return rc;
        if ((rc = ensure_cap(c, c->d_tmat_H, n2))) return rc;
        cplx** base = p->kind == SK_CONST ? &p->d_hbase : &c->d_F;
        NEGF_HIP_CHECK(hipMemcpyAsync(c->d_tmat_H.p, *base, n2 * sizeof(cplx), hipMemcpyDeviceToDevice, c->stream));
        launch_tmat_add_probes(c->stream, n, n_probes, r->d_order, dK, r->d_ioff, r->d_soff, r->d_idx, c->d_tmat_sig, c->d_tmat_H);
        launch_tmat_gamma(c->stream, nc, n_probes, 1, dK, r->d_soff, r->d_goff, r->d_gstride, c->d_tmat_sig, 0, r->gam);
        r->swap.set(base, c->d_tmat_H.p);
    }
    if (!pl.per_energy) launch_tmat_gamma(c->stream, 0, nc, 1, dK, r->d_soff, r->d_goff, r->d_gstride, p->d_const_blk, 0, r->gam);
    return NEGF_OK;
}

// the batch [m0, m0 + nb): assemble + inverse (c->G), the contacts' Gamma blocks of a block provider, and -- T != nullptr --
// the pair / product sequence into T [nb][C][C], NaN for singular energies
int tmat_batch(negf_ctx* c, SigmaProvider* p, const TmatRun& r, int m0, int nb, const cplx* E, double* T)
{
    int rc;
    const TmatPlan& pl = r.pl;
    const int n = c->n, C = pl.C, nc = pl.nc;
    const size_t n2 = (size_t)n * n, C2 = (size_t)C * C;
    if ((rc = run_assemble_inverse(c, p, m0, nb, E))) return rc;
    ProfScope ps(c, "tmat");
    if (pl.per_energy)
        launch_tmat_gamma(c->stream, 0, nc, nb, r.dK, r.d_soff, r.d_goff, r.d_gstride, c->d_blk, (size_t)p->blk_stride, r.gam);
    if (!T) return NEGF_OK;
    double cmadds = 0;
    for (int cls = 1; cls <= 2; ++cls) {
        launch_tmat_pairs(c->stream, cls, n, C, (int)pl.pairs[cls].size(), pl.max_elems[cls], nb,
                          c->d_tmat_tab.p + r.pair_at[cls], r.dK, r.d_ioff, r.d_goff, r.d_gstride, r.d_idx, c->G, r.gam, T);
        for (int pr : pl.pairs[cls]) {
            const double ka = pl.K[pr / C], kb = pl.K[pr % C];
            cmadds += ka * kb * (ka + kb);
        }
    }
    negf_count_flops(8.0 * cmadds * nb, 0.0);
    // pairs of two lead-sized blocks (and blocks beyond the LDS of the pair kernel): G_ab gathered, X = Gamma_a G_ab,
    // Y = X Gamma_b on the matrix cores, T = Re sum Y conj(G_ab)
    for (int pr : pl.pairs[0]) {
        const int a = pr / C, b = pr - a * C, Ka = pl.K[a], Kb = pl.K[b];
        const size_t kk = (size_t)Ka * Kb;
        cplx* Gab = c->d_tmat_work;
        launch_gather_block(c->stream, n, Ka, Kb, nb, c->G, n2, r.d_idx + pl.ioff[a], r.d_idx + pl.ioff[b], Gab, kk);
        launch_zgemm(c->stream, Ka, Kb, Ka, nb, r.gam + pl.goff[a], Ka, (size_t)pl.gstride[a], Gab, Kb, kk, 0, c->W1, Kb, n2);
        launch_zgemm(c->stream, Ka, Kb, Kb, nb, c->W1, Kb, n2, r.gam + pl.goff[b], Kb, (size_t)pl.gstride[b], 0, c->W2, Kb, n2);
        launch_trace_dot(c->stream, Ka, Kb, nb, c->W2, Kb, n2, Gab, Kb, kk, T + (size_t)a * C + b, (int)C2);
    }
    launch_tmat_nan(c->stream, C, nb, c->d_info + m0, T);
    return NEGF_OK;
}

// R [nb][P][n_c] of the batch whose matrices are in T [nb][C][C] (d_order: the probes' terminal numbers in the order of
// the rows of W); the global class of the response kernel goes through in chunks
// of as many energies as its work area holds
int deph_run_response(negf_ctx* c, int C, int nc, const int* d_order, int nb, const double* T, double* R)
{
    const int P = C - nc;
    if (P <= 0 || nc <= 0) return NEGF_OK;
    const size_t per = deph_response_work_doubles(P, nc);
    int chunk = nb;
    if (per > 0) {
        chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, DEPH_WORK_BYTES / (per * sizeof(double))));
        if (int rc = ensure_cap(c, c->d_deph_work, per * chunk)) return rc;
    }
    ProfScope ps(c, "deph");
    for (int b0 = 0; b0 < nb; b0 += chunk)
        launch_deph_response(c->stream, C, nc, std::min(chunk, nb - b0), d_order, T + (size_t)b0 * C * C, c->d_deph_work,
                             R + (size_t)b0 * P * nc);
    return NEGF_OK;
}

}  // namespace

int negf_transmission_matrix_dev(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                                 const double* probe_sigma, int m, const double* E_dev, double* T_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    TmatRun run;
    if ((rc = tmat_plan(c, p, n_probes, probe_nk, probe_inds, reinterpret_cast<const cplx*>(probe_sigma), &run.pl))) return rc;
    if (m > 0 && (!E_dev || !T_dev)) return NEGF_EINVAL;
    if (m == 0) { c->last_m = 0; return NEGF_OK; }
    const size_t C2 = (size_t)run.pl.C * run.pl.C;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    return dense_batches(c, p, m, [&](int) { return tmat_setup(c, p, &run); },
                         [&](int m0, int nb) { return tmat_batch(c, p, run, m0, nb, E, T_dev + C2 * m0); });
}

int negf_transmission_matrix(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                             const double* probe_sigma, int m, const double* E, double* T, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!probes_count_ok(p, n_probes) || (m > 0 && (!E || !T))) return NEGF_EINVAL;
    const size_t C = (size_t)p->n_contacts + n_probes, cnt = (size_t)m * C * C;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_bond_T, cnt))) return rc;
    if ((rc = negf_transmission_matrix_dev(c, handle, n_probes, probe_nk, probe_inds, probe_sigma, m,
                                           dev_E(c), c->d_bond_T))) return rc;
    return fetch_pageable(c, m, {{T, c->d_bond_T.p, cnt}}, info);
}

// ------------------------------------------------- floating dephasing probes: response, G^<, G^r
// The probes of negf_transmission_matrix left floating at every energy (k_dephase.hip): their response R to the real
// contacts from the transmission matrices of the batch, and the lesser Green's function's weighted sum with the
// dephased coupling D_s = Gamma_s + sum_p R_ps Gamma_p in the place of Gamma_s -- one inverse per energy, nothing
// crosses to the host.  The reference has no such function.
int negf_probe_response_dev(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                            const double* probe_sigma, int m, const double* E_dev, double* R_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    TmatRun run;
    if ((rc = tmat_plan(c, p, n_probes, probe_nk, probe_inds, reinterpret_cast<const cplx*>(probe_sigma), &run.pl))) return rc;
    if (m > 0 && (!E_dev || (n_probes > 0 && !R_dev))) return NEGF_EINVAL;
    if (m == 0) { c->last_m = 0; return NEGF_OK; }
    const size_t C2 = (size_t)run.pl.C * run.pl.C, pc = (size_t)n_probes * run.pl.nc;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    auto setup = [&](int batch) {
        if (int e = tmat_setup(c, p, &run)) return e;
        return ensure_cap(c, c->d_deph_T, C2 * batch);
    };
    return dense_batches(c, p, m, setup, [&](int m0, int nb) {
        if (int e = tmat_batch(c, p, run, m0, nb, E, c->d_deph_T)) return e;
        return deph_run_response(c, run.pl.C, run.pl.nc, run.d_order, nb, c->d_deph_T, R_dev + pc * m0);
    });
}

int negf_probe_response(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                        const double* probe_sigma, int m, const double* E, double* R, int* info)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    if (!probes_count_ok(p, n_probes) || (m > 0 && (!E || (n_probes > 0 && !R)))) return NEGF_EINVAL;
    const size_t cnt = (size_t)m * n_probes * p->n_contacts;
    if ((rc = stage_grid(c, m, p->n_contacts, E, nullptr)) || (rc = ensure_cap(c, c->d_deph_R, cnt))) return rc;
    if ((rc = negf_probe_response_dev(c, handle, n_probes, probe_nk, probe_inds, probe_sigma, m,
                                      dev_E(c), c->d_deph_R))) return rc;
    return fetch_pageable(c, m, {{R, c->d_deph_R.p, cnt}}, info);
}

int negf_gless_int_probes_dev(negf_ctx* c, int handle, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                              const double* probe_sigma, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    SigmaProvider* p;
    int contact;
    int rc = open_call(c, handle, m, &p, ind, &contact);
    if (rc) return rc;
    TmatRun run;
    if ((rc = tmat_plan(c, p, n_probes, probe_nk, probe_inds, reinterpret_cast<const cplx*>(probe_sigma), &run.pl))) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    const int n = c->n;
    const size_t n2 = (size_t)n * n;
    cplx* out = reinterpret_cast<cplx*>(out_dev);
    if (m == 0) {
        NEGF_HIP_CHECK(hipMemsetAsync(out, 0, n2 * sizeof(cplx), c->stream));
        c->last_m = 0;
        return NEGF_OK;
    }
    const TmatPlan& pl = run.pl;
    const int C = pl.C, nc = pl.nc;
    const bool floating = contact >= 0 && n_probes > 0;        // the total needs no response: every weight is 1
    // the terminals that enter D, in the order they are added: the contact(s), then the probes in content order
    std::vector<int> list;
    if (contact >= 0) list.push_back(contact);
    else for (int t = 0; t < nc; ++t) list.push_back(t);
    list.insert(list.end(), pl.order.begin(), pl.order.end());
    // U = the sorted union of their orbitals; the compact products when 2 K_U <= n, otherwise U = all orbitals and D is n x n
    std::vector<int> where(n, -1), U;
    for (int t : list)
        for (int i = 0; i < pl.K[t]; ++i) where[pl.idx[pl.ioff[t] + i]] = 0;
    for (int i = 0; i < n; ++i) if (where[i] == 0) U.push_back(i);
    const bool compact = 2 * U.size() <= (size_t)n;
    if (!compact) { U.resize(n); for (int i = 0; i < n; ++i) U[i] = i; }
    const int KU = (int)U.size();
    for (int k = 0; k < KU; ++k) where[U[k]] = k;
    std::vector<int> tab(U);
    for (int v : pl.idx) tab.push_back(where[v]);
    tab.insert(tab.end(), list.begin(), list.end());
    const int *d_U = nullptr, *d_pos = nullptr, *d_list = nullptr;
    const cplx* E = reinterpret_cast<const cplx*>(E_dev);
    const cplx* w = reinterpret_cast<const cplx*>(w_dev);
    // behind the transmission matrix's set-up: the tables, the per-batch areas of the response and of D, out cleared
    auto setup = [&](int batch) {
        int e;
        if ((e = tmat_setup(c, p, &run))) return e;
        if ((e = ensure_cap(c, c->d_deph_tab, tab.size())) || (e = upload(c, c->d_deph_tab.p, tab.data(), tab.size()))) return e;
        d_U = c->d_deph_tab;
        d_pos = d_U + KU;
        d_list = d_pos + pl.idx.size();
        if (floating) {
            if ((e = ensure_cap(c, c->d_deph_T, (size_t)C * C * batch))) return e;
            if ((e = ensure_cap(c, c->d_deph_R, (size_t)n_probes * nc * batch))) return e;
        }
        if (compact && (e = ensure_cap(c, c->d_deph_D, (size_t)KU * KU * batch))) return e;
        if (batch < m && (e = ensure_cap(c, c->d_deph_carry, n2))) return e;      // (a grid in one batch carries nothing)
        return clear_first(c, out, n2 * sizeof(cplx))(batch);
    };
    return dense_batches(c, p, m, setup, [&](int m0, int nb) {
        int e;
        if ((e = tmat_batch(c, p, run, m0, nb, E, floating ? c->d_deph_T.p : nullptr))) return e;
        if (floating && (e = deph_run_response(c, C, nc, run.d_order, nb, c->d_deph_T, c->d_deph_R))) return e;
        cplx* D = compact ? c->d_deph_D.p : c->W1;
        const size_t sD = compact ? (size_t)KU * KU : n2;
        {
            ProfScope ps(c, "deph");
            launch_deph_coupling(c->stream, KU, nc, n_probes, floating ? contact : -1, (int)list.size(), nb, d_list, run.dK,
                                 run.d_ioff, run.d_goff, run.d_gstride, d_pos, run.gam, c->d_deph_R, D, sD);
        }
        { ProfScope ps(c, "zgemm"); launch_g_d_gh(c, nb, KU, compact ? d_U : nullptr, D, sD); }      // as run_gless_products
        ProfScope ps(c, "accumulate");
        // (the grid's 32-energy chunks, not the batch's: the bits do not depend on the batch -- launch_bond_int's order)
        launch_accumulate_grid(c->stream, (int)n2, m, m0, nb, w + m0, c->W1, c->d_deph_carry, c->W2, out);
        return NEGF_OK;
    });
}

int negf_gless_int_probes(negf_ctx* c, int handle, int ind, int n_probes, const int* probe_nk, const int* probe_inds,
                          const double* probe_sigma, int m, const double* E, const double* w, double* out, int* info)
{
    return host_integral(c, handle, n_probes, m, E, w, out, info, [&](double* Ed, double* wd, double* acc) {
        return negf_gless_int_probes_dev(c, handle, ind, n_probes, probe_nk, probe_inds, probe_sigma, m, Ed, wd, acc);
    });
}

// sum_k w_k G(E_k) with the probes in A: negf_gr_int_dev's pass while the copy of F that carries the probes stands in
int negf_gr_int_probes_dev(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                           const double* probe_sigma, int m, const double* E_dev, const double* w_dev, double* out_dev)
{
    SigmaProvider* p;
    int rc = open_call(c, handle, m, &p);
    if (rc) return rc;
    TmatRun run;
    if ((rc = tmat_plan(c, p, n_probes, probe_nk, probe_inds, reinterpret_cast<const cplx*>(probe_sigma), &run.pl))) return rc;
    if (!out_dev || (m > 0 && (!E_dev || !w_dev))) return NEGF_EINVAL;
    // (negf_gr_int_dev's pass, small path included, behind the set-up of a transmission-matrix call)
    if (m > 0 && ((rc = ensure_mbuffers(c, m, p->n_contacts)) || (rc = ensure_workspace(c, m, p->blk_stride)) ||
                  (rc = tmat_setup(c, p, &run)))) return rc;
    return negf_gr_int_dev(c, handle, m, E_dev, w_dev, out_dev);
}

int negf_gr_int_probes(negf_ctx* c, int handle, int n_probes, const int* probe_nk, const int* probe_inds,
                       const double* probe_sigma, int m, const double* E, const double* w, double* out, int* info)
{
    return host_integral(c, handle, n_probes, m, E, w, out, info, [&](double* Ed, double* wd, double* acc) {
        return negf_gr_int_probes_dev(c, handle, n_probes, probe_nk, probe_inds, probe_sigma, m, Ed, wd, acc);
    });
}

// ------------------------------------------------------------ g(E) cache knob
int negf_set_chain_cache(negf_ctx* c, int max_grids)
{
    if (!c || max_grids < 0 || max_grids > 4096) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (max_grids < (int)c->gcache.size()) free_gcache(c);     // shrinking (or switching off) drops every entry
    c->gcache_max = max_grids;
    c->gcache.reserve((size_t)max_grids);                      // entries are handed out by pointer: no reallocation later
    return NEGF_OK;
}

int negf_set_chain_cache_bytes(negf_ctx* c, long long max_bytes)
{
    if (!c || max_bytes < 0) return NEGF_EINVAL;
    c->gcache_bytes_max = (size_t)max_bytes;
    return NEGF_OK;
}

int negf_chain_cache_clear(negf_ctx* c)
{
    if (!c) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    NEGF_HIP_CHECK(hipStreamSynchronize(c->stream));
    free_gcache(c);
    c->gcache.reserve((size_t)c->gcache_max);
    return NEGF_OK;
}

int negf_chain_cache_stats(negf_ctx* c, long long* hits, long long* misses, long long* entries, long long* bytes)
{
    if (!c) return NEGF_EINVAL;
    long long n = 0, b = 0;
    for (const auto& e : c->gcache)
        if (e.valid) { ++n; b += (long long)(e.g_cap * sizeof(cplx) + 2 * e.it_cap * sizeof(int)); }
    if (hits) *hits = (long long)c->gcache_hits;
    if (misses) *misses = (long long)c->gcache_misses;
    if (entries) *entries = n;
    if (bytes) *bytes = b;
    return NEGF_OK;
}

// ------------------------------------------------------------------ diagnostics
int negf_workspace_bytes(negf_ctx* c, long long* work, long long* blocks)
{
    if (!c) return NEGF_EINVAL;
    if (work) *work = c->batch > 0 ? 3LL * ((long long)c->n * c->n * c->batch + 64) * (long long)sizeof(cplx) : 0;
    if (blocks) *blocks = (long long)c->d_blk.cap * (long long)sizeof(cplx);
    return NEGF_OK;
}

int negf_profile_enable(negf_ctx* c, int on) { if (!c) return NEGF_EINVAL; c->profiling = on != 0; return NEGF_OK; }
int negf_profile_reset(negf_ctx* c) { if (!c) return NEGF_EINVAL; prof_resolve(c); c->prof.clear(); return NEGF_OK; }
int negf_profile_read(negf_ctx* c, const char* family, double* total_ms, int* launches)
{
    if (!c || !family) return NEGF_EINVAL;
    prof_resolve(c);
    auto it = c->prof.find(family);
    if (total_ms) *total_ms = it == c->prof.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->prof.end() ? 0 : it->second.launches;
    return NEGF_OK;
}

int negf_profile_read_flops(negf_ctx* c, const char* family, double* flops_algorithmic, double* flops_mfma_issued)
{
    if (!c || !family) return NEGF_EINVAL;
    auto it = c->prof.find(family);
    if (flops_algorithmic) *flops_algorithmic = it == c->prof.end() ? 0.0 : it->second.flops_alg;
    if (flops_mfma_issued) *flops_mfma_issued = it == c->prof.end() ? 0.0 : it->second.flops_mfma;
    return NEGF_OK;
}

int negf_selftest_mfma(negf_ctx* c, double* max_err)
{
    if (!c || !max_err) return NEGF_EINVAL;
    NEGF_HIP_CHECK(hipSetDevice(c->device));
    return run_mfma_selftest(c->stream, max_err);
}

}  // extern "C"

// the layered (recursive Green's function) entry points: negf_layered_*
#include "negf_layered_impl.h"
