// slices_eval.inc -- slice-level correctness and AUC1 of slice searches (included by knn355_lib.hip behind assemble.inc).
//
// The reference judges the hits of pfam/slices/slices_search.py in Python loops under tqdm: per slice the Pfam domains
// of its protein that lie inside the slice or merely intersect it (pfam/slices/slices.py:49-68), the family sizes
// (:70-74), the slices with exactly one family inside (:76-80), and then evaluate (:101-142): per annotated query slice
// and hit two set look-ups, and a run over the row that counts correct hits, skips ignored ones and ends at the first
// hit that is neither.  The contract is above knn_eval_slice_annotate and knn_eval_slices in include/knn355.h.
//
// No set is materialised.  The domains of a protein are sorted by family, so "family a has a domain inside slice h" is
// a lower-bound search for a in the protein's range and the interval tests over a's run of equal codes.
//
//   slice_annotate_kernel  one thread per slice walks its protein's domains in family order; a family counts once, at
//                          the first inside domain of its run (one "last family counted" register).  family_sizes is
//                          filled by 64-bit integer atomics: the sum does not depend on their order.
//   slice_eval_kernel      one wave per row of hits, four rows per workgroup, the row walked 64 hits at a time.  Per hit
//                          one 16-byte load of the hit slice's record {protein, start, stop, match_count}, the search,
//                          the tests.  __ballot gives the chunk's correct mask and its stop mask (neither correct nor
//                          ignored); lead is the popcount of correct below the first stop bit, carried across chunks
//                          while no stop bit has been seen; tp adds the popcounts; column_correct takes one integer
//                          atomic per correct hit.
//
// Where this departs from the shape the kernels were first sketched in: the domain table is packed on the host too,
// into one 16-byte record {family, start, stop, 0} per domain, so the search and the interval tests of a hit read the
// same line instead of three arrays; and the annotate kernel walks the slices with a grid-stride loop, so the grid stays
// small whatever ns is.

__global__ __launch_bounds__(256) void slice_annotate_kernel(const int32_t *__restrict__ slice_protein, const int32_t *__restrict__ slice_start,
                                                             const int32_t *__restrict__ slice_stop, int64_t ns,
                                                             const int64_t *__restrict__ doff, const int4 *__restrict__ dom,
                                                             int32_t *__restrict__ match_count, int32_t *__restrict__ annotation,
                                                             unsigned long long *__restrict__ family_sizes)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += stride) {
        const int32_t p = slice_protein[s];
        int32_t cnt = 0, last = -1;
        if (p >= 0) {
            const int32_t s0 = slice_start[s], s1 = slice_stop[s];
            const int64_t hi = doff[p + 1];
            for (int64_t d = doff[p]; d < hi; d++) {
                const int4 r = dom[d];
                if (r.x != last && s0 <= r.y && r.z <= s1) {
                    last = r.x;
                    cnt++;
                    atomicAdd(&family_sizes[r.x], 1ull);
                }
            }
        }
        match_count[s] = cnt;
        annotation[s] = cnt == 1 ? last : -1;
    }
}

__global__ __launch_bounds__(256) void slice_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int32_t *__restrict__ query_family,
                                                         const int4 *__restrict__ rec, int64_t ns, const int64_t *__restrict__ doff,
                                                         const int4 *__restrict__ dom, int ignore_unannotated,
                                                         uint8_t *__restrict__ is_correct, uint8_t *__restrict__ is_ignore,
                                                         int32_t *__restrict__ lead, int32_t *__restrict__ tp,
                                                         unsigned long long *__restrict__ column_correct)
{
    int lane;
    int64_t r;
    if (!wave_row(nq, lane, r)) return;
    const int32_t a = query_family[r];
    const int64_t *h = hits + r * k;
    uint8_t *ic = is_correct + r * k, *ig = is_ignore + r * k;
    int lead_n = 0, tp_n = 0;
    bool open = true; // no stop hit so far
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int j = c0 + lane;
        const bool in = j < k;
        bool correct = false, ignore = false;
        if (in && a >= 0) {
            const int64_t hid = h[j];
            if (hid >= 0 && hid < ns) {
                const int4 s = rec[hid];
                ignore = ignore_unannotated && s.w == 0;
                if (s.x >= 0) {
                    const int64_t hi = doff[s.x + 1];
                    // (the protein's domains are sorted by family: the run of family a starts at its lower bound)
                    for (int64_t d = lower_bound_dev(doff[s.x], hi, [&](int64_t i) { return dom[i].x < a; }); d < hi; d++) {
                        const int4 m = dom[d];
                        if (m.x != a) break;
                        if (s.y <= m.y && m.z <= s.z) correct = true;
                        else if (s.y < m.z && m.y < s.z) ignore = true;
                    }
                }
            }
        }
        if (in) {
            ic[j] = correct ? 1 : 0;
            ig[j] = ignore ? 1 : 0;
        }
        const uint64_t cm = __ballot(correct), sm = __ballot(in && !correct && !ignore);
        tp_n += __builtin_popcountll(cm);
        if (open) {
            if (sm) {
                lead_n += __builtin_popcountll(cm & ((1ull << __builtin_ctzll(sm)) - 1ull));
                open = false;
            } else {
                lead_n += __builtin_popcountll(cm);
            }
        }
        if (column_correct && correct) atomicAdd(&column_correct[j], 1ull);
    }
    if (lane == 0) {
        lead[r] = lead_n;
        tp[r] = tp_n;
    }
}

// the tables both entry points take: everything the kernels rely on without further checks
static int slices_check_tables(const char *who, const int32_t *slice_protein, const int32_t *slice_start, const int32_t *slice_stop,
                               int64_t ns, const int64_t *domain_offsets, const int32_t *domain_family, const int32_t *domain_start,
                               const int32_t *domain_stop, int64_t np, int64_t nfam)
{
    const std::string w(who);
    if (ns > 0 && (!slice_protein || !slice_start || !slice_stop)) return set_err(KNN_ERR_INVALID, w + ": null pointer");
    if (np > 0 && !domain_offsets) return set_err(KNN_ERR_INVALID, w + ": null pointer");
    if (np > (int64_t)INT32_MAX) return set_err(KNN_ERR_INVALID, w + ": np > INT32_MAX");
    int64_t nd = 0;
    if (np > 0) {
        EVAL_TRY(eval_check_offsets(w, "domain", domain_offsets, np));
        nd = domain_offsets[np];
    }
    if (nd > 0 && (!domain_family || !domain_start || !domain_stop)) return set_err(KNN_ERR_INVALID, w + ": null pointer");
    for (int64_t p = 0; p < np; p++)
        for (int64_t d = domain_offsets[p]; d < domain_offsets[p + 1]; d++) {
            if (domain_family[d] < 0 || domain_family[d] >= nfam) return set_err(KNN_ERR_INVALID, w + ": domain family outside [0, nfam)");
            if (d > domain_offsets[p] && domain_family[d] < domain_family[d - 1])
                return set_err(KNN_ERR_INVALID, w + ": domain families of a protein not sorted");
        }
    for (int64_t s = 0; s < ns; s++)
        if (slice_protein[s] < -1 || slice_protein[s] >= np) return set_err(KNN_ERR_INVALID, w + ": slice protein outside [-1, np)");
    return 0;
}

// the domain tables as columns of the whole-call walker: the offsets, and {family, start, stop, 0} per domain packed into
// `packed`, which the caller keeps until the upload (np == 0: no slice has a protein, nothing reads either)
static void slices_domain_columns(EvalCols &tab, const int64_t *domain_offsets, const int32_t *domain_family, const int32_t *domain_start,
                                  const int32_t *domain_stop, int64_t np, std::vector<int4> &packed, const int64_t **d_off,
                                  const int4 **d_dom)
{
    const int64_t nd = np > 0 ? domain_offsets[np] : 0, d0 = np > 0 ? domain_offsets[0] : 0;
    packed.assign((size_t)nd, make_int4(0, 0, 0, 0));
    for (int64_t d = d0; d < nd; d++) packed[(size_t)d] = make_int4(domain_family[d], domain_start[d], domain_stop[d], 0);
    *d_off = tab.in(np > 0 ? domain_offsets : nullptr, (size_t)(np + 1) * 8);
    *d_dom = tab.in(packed.data(), (size_t)nd * 16);
}

extern "C" int knn_eval_slice_annotate(const int32_t *slice_protein, const int32_t *slice_start, const int32_t *slice_stop, int64_t ns,
                                       const int64_t *domain_offsets, const int32_t *domain_family, const int32_t *domain_start,
                                       const int32_t *domain_stop, int64_t np, int64_t nfam, int32_t *match_count, int32_t *annotation,
                                       int64_t *family_sizes)
{
    if (ns < 0 || np < 0 || nfam < 0) return set_err(KNN_ERR_INVALID, "slice_annotate: negative ns, np or nfam");
    if ((ns > 0 && (!match_count || !annotation)) || (nfam > 0 && !family_sizes)) return set_err(KNN_ERR_INVALID, "slice_annotate: null pointer");
    int rc = slices_check_tables("slice_annotate", slice_protein, slice_start, slice_stop, ns, domain_offsets, domain_family, domain_start,
                                 domain_stop, np, nfam);
    if (rc) return rc;
    if (ns == 0) { // no slice holds any family
        for (int64_t f = 0; f < nfam; f++) family_sizes[f] = 0;
        return 0;
    }
    rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    EvalCols tab(bufs, 1), w(bufs, ns); // (the slices go in one slab: a slice is 12 bytes in and 8 out)
    std::vector<int4> packed;
    const int64_t *d_off;
    const int4 *d_dom;
    slices_domain_columns(tab, domain_offsets, domain_family, domain_start, domain_stop, np, packed, &d_off, &d_dom);
    unsigned long long *d_fs = (unsigned long long *)tab.out(family_sizes, (size_t)nfam * 8);
    const int32_t *d_sp = w.in(slice_protein, 4);
    const int32_t *d_s0 = w.in(slice_start, 4);
    const int32_t *d_s1 = w.in(slice_stop, 4);
    int32_t *d_mc = w.out(match_count, 4);
    int32_t *d_an = w.out(annotation, 4);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    EVAL_TRY(w.upload(0, ns));
    if (nfam) HIP_TRY(hipMemset(d_fs, 0, (size_t)nfam * 8));
    const unsigned grid = (unsigned)std::min<int64_t>((ns + 255) / 256, 8192);
    hipLaunchKernelGGL(slice_annotate_kernel, dim3(grid), dim3(256), 0, 0, d_sp, d_s0, d_s1, ns, d_off, d_dom, d_mc, d_an, d_fs);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(w.download(0, ns));
    EVAL_TRY(tab.download(0, 1));
    return 0;
}

extern "C" int knn_eval_slices(const int64_t *hits, int64_t nq, int64_t k, const int32_t *query_family, const int32_t *slice_protein,
                               const int32_t *slice_start, const int32_t *slice_stop, int64_t ns, const int64_t *domain_offsets,
                               const int32_t *domain_family, const int32_t *domain_start, const int32_t *domain_stop, int64_t np,
                               int64_t nfam, const int32_t *match_count, int32_t ignore_unannotated, uint8_t *is_correct,
                               uint8_t *is_ignore, int32_t *lead, int32_t *tp, int64_t *column_correct)
{
    if (nq < 0 || ns < 0 || np < 0 || nfam < 0) return set_err(KNN_ERR_INVALID, "eval_slices: negative nq, ns, np or nfam");
    if (k < 1) return set_err(KNN_ERR_INVALID, "eval_slices: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "eval_slices: k > INT32_MAX");
    if (nq == 0) return 0;
    if (!hits || !query_family || !is_correct || !is_ignore || !lead || !tp || (ignore_unannotated && ns > 0 && !match_count))
        return set_err(KNN_ERR_INVALID, "eval_slices: null pointer");
    for (int64_t q = 0; q < nq; q++)
        if (query_family[q] >= nfam) return set_err(KNN_ERR_INVALID, "eval_slices: query family >= nfam");
    int rc = slices_check_tables("eval_slices", slice_protein, slice_start, slice_stop, ns, domain_offsets, domain_family, domain_start,
                                 domain_stop, np, nfam);
    if (rc) return rc;
    if (ns == 0) { // every hit is outside the table: nothing is correct, nothing ignored
        memset(is_correct, 0, (size_t)nq * k);
        memset(is_ignore, 0, (size_t)nq * k);
        for (int64_t q = 0; q < nq; q++) lead[q] = tp[q] = 0;
        if (column_correct)
            for (int64_t j = 0; j < k; j++) column_correct[j] = 0;
        return 0;
    }
    rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EvalCols tab(bufs, 1), w(bufs, slab);
    std::vector<int4> packed, recs((size_t)ns);
    for (int64_t s = 0; s < ns; s++)
        recs[(size_t)s] = make_int4(slice_protein[s], slice_start[s], slice_stop[s], match_count ? match_count[s] : 0);
    const int64_t *d_off;
    const int4 *d_dom;
    slices_domain_columns(tab, domain_offsets, domain_family, domain_start, domain_stop, np, packed, &d_off, &d_dom);
    const int4 *d_rec = tab.in(recs.data(), (size_t)ns * 16);
    unsigned long long *d_cc = (unsigned long long *)tab.out(column_correct, (size_t)k * 8);
    const int64_t *d_h = w.in(hits, (size_t)k * 8);
    const int32_t *d_qf = w.in(query_family, 4);
    uint8_t *d_ic = w.out(is_correct, (size_t)k);
    uint8_t *d_ig = w.out(is_ignore, (size_t)k);
    int32_t *d_lead = w.out(lead, 4);
    int32_t *d_tp = w.out(tp, 4);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    if (d_cc) HIP_TRY(hipMemset(d_cc, 0, (size_t)k * 8));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(slice_eval_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_qf, d_rec, ns, d_off, d_dom,
                           ignore_unannotated ? 1 : 0, d_ic, d_ig, d_lead, d_tp, d_cc);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    EVAL_TRY(tab.download(0, 1));
    return 0;
}
