// --- Leaf regularisation (DESIGN.md section 11, "Leaf regularisation"; host side: lambdamart_reg.hpp) ---------------------
// lambda_l1, max_delta_step, path_smooth (Newton gain only): a side's output is no longer G / (H + lambda_l2) clamped to an
// interval but, in this order, the soft-thresholded gradient sum T over den = H + lambda_l2 (q0), capped at +-max_delta_step,
// pulled toward the parent's output p by r = n / path_smooth ((o r) / (r + 1) + p / (r + 1)), and clamped to [lo, hi]; a side
// whose output stayed at q0 has the term (T T) / den, a moved one (2 T) v - (den v) v.  Every operation is rounded on its own.
// The records are the Newton kernels'; validity is the monotone kernels' (the order of vL, vR under a sign included).  The
// kernels of kernels_hist.inc keep their code; these stand next to them and run only when one of the three keys is set,
// with or without monotone signs (sign[] may be all zero).
//
//   hist_scan_reg_kernel       hist_scan_monotone_kernel with reg[node] = {lo, hi, parent, has_parent}: the node's own output
//                              comes from its totals under that record, and both sides of a candidate are pulled toward it
//   hist_leaf_scan_reg_kernel  hist_leaf_scan_monotone_kernel with one such record per child
//   hist_scan_sym_reg_kernel / hist_sym_apply_reg_kernel
//                              the symmetric pair under lambda_l1 / max_delta_step (no parent, no interval)

// the three numbers next to the Newton gain's
struct HistRegDev {
    double l1, l2, mds, smooth, min_hess;
};
// a node's interval, its parent's output and whether it has a parent
struct HistRegNodeDev {
    double lo, hi, parent;
    uint32_t has_parent, pad;
};
// the same of the (at most two) children a leaf-wise step scans
struct HistLeafRegDev {
    double lo[2], hi[2], parent[2];
    uint32_t has_parent[2];
};

// term of one side (n instances) of a candidate; *v: its output.  Every form is computed and one is selected: the lanes of a
// wave disagree about which case they are in
__device__ __forceinline__ double hist_reg_term(long long q, double h, uint32_t n, int s_l, const HistRegDev& p, double lo, double hi, double parent,
                                                bool has_parent, double* v) {
    const double g = ldexp((double)q, -s_l), den = h + p.l2;
    const double t = g > p.l1 ? g - p.l1 : (g < -p.l1 ? g + p.l1 : 0.0);
    const double quot = t / den;
    const double q0 = den != 0.0 ? quot : 0.0;
    double capped = q0 > p.mds ? p.mds : q0;
    capped = capped < -p.mds ? -p.mds : capped;
    double o = p.mds > 0.0 ? capped : q0;
    const double r = (double)n / p.smooth;
    const double smoothed = (o * r) / (r + 1.0) + parent / (r + 1.0);
    o = (p.smooth > 0.0 && has_parent) ? smoothed : o;
    double c = o < lo ? lo : o;
    c = c > hi ? hi : c;
    const double plain = (t * t) / den;
    const double moved = (2.0 * t) * c - (den * c) * c;
    *v = c;
    return c == q0 ? plain : moved;
}

// (validity as hist_monotone_candidate's; false: no candidate).  vnode: the splitting node's own output, both sides' parent
__device__ __forceinline__ bool hist_reg_candidate(uint32_t nl, uint32_t nr, long long ql, long long wl, long long qtot, long long wtot, int s_l,
                                                   int s_w, const HistRegDev& p, double lo, double hi, double vnode, int sign, double* imp) {
    const double hl = ldexp((double)wl, -s_w), hr = ldexp((double)(wtot - wl), -s_w);
    if (!(hl >= p.min_hess && hr >= p.min_hess && hl + p.l2 > 0.0 && hr + p.l2 > 0.0)) return false;
    double vl, vr;
    const double tl = hist_reg_term(ql, hl, nl, s_l, p, lo, hi, vnode, true, &vl);
    const double tr = hist_reg_term(qtot - ql, hr, nr, s_l, p, lo, hi, vnode, true, &vr);
    if ((sign > 0 && !(vl <= vr)) || (sign < 0 && !(vl >= vr))) return false;
    *imp = tl + tr;
    return true;
}

// one wave per (node, feature), as hist_scan_monotone_kernel.  reg[a]: node a's record
__global__ __launch_bounds__(64) void hist_scan_reg_kernel(const HistItemDev* __restrict__ nodes, const HistRegNodeDev* __restrict__ reg, uint32_t F,
                                                           uint32_t k, const uint32_t* __restrict__ nedges, const int* __restrict__ sign,
                                                           const uint32_t* __restrict__ fsel, const uint32_t* __restrict__ cnt,
                                                           const unsigned long long* __restrict__ sum, const unsigned long long* __restrict__ wsum,
                                                           uint32_t min_leaf, int s_l, int s_w, HistRegDev p, HistBestNewtonDev* __restrict__ best) {
    const uint32_t a = blockIdx.x / F, f = blockIdx.x % F, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const HistRegNodeDev rg = reg[a];
    const bool has_parent = rg.has_parent != 0;
    const uint32_t n = nd.end - nd.begin;
    const uint32_t row = fsel ? fsel[f] : f;
    const uint32_t ne = min(nedges[row], k - 1);
    const int sg = sign[row];
    const size_t base = ((size_t)nd.slot * F + f) * k;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = in ? (long long)wsum[base + b] : 0ll;
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    double vnode;  // the node's own output: what both sides are pulled toward
    (void)hist_reg_term(qtot, ldexp((double)wtot, -s_w), n, s_l, p, rg.lo, rg.hi, rg.parent, has_parent, &vnode);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        double imp;
        if (!hist_reg_candidate(nl, nr, rs, rw, qtot, wtot, s_l, s_w, p, rg.lo, rg.hi, vnode, sg, &imp)) continue;
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistBestNewtonDev* out = best + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistBestNewtonDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, 0u};
    } else if (have && bj == wj) {
        *out = HistBestNewtonDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, 0u};
    }
}

// grid (F, children), as hist_leaf_scan_monotone_kernel: the in-place parent - sibling derivation, then the scan under the
// child's own record.  rec[child * F + f]
__global__ __launch_bounds__(64) void hist_leaf_scan_reg_kernel(HistLeafKids kids, HistLeafRegDev reg, uint32_t F, uint32_t k,
                                                                const uint32_t* __restrict__ nedges, const int* __restrict__ sign,
                                                                const uint32_t* __restrict__ fsel, uint32_t* cnt, unsigned long long* sum,
                                                                unsigned long long* wsum, uint32_t min_leaf, int s_l, int s_w, HistRegDev p,
                                                                HistPickDev* __restrict__ rec) {
    const uint32_t f = blockIdx.x, a = blockIdx.y, lane = threadIdx.x;
    const uint32_t n = kids.n[a];
    const double lo = reg.lo[a], hi = reg.hi[a], parent = reg.parent[a];
    const bool has_parent = reg.has_parent[a] != 0;
    const uint32_t row = fsel ? fsel[f] : f;
    const uint32_t ne = min(nedges[row], k - 1);
    const int sg = sign[row];
    const size_t base = ((size_t)kids.slot[a] * F + f) * k, obase = ((size_t)kids.other[a] * F + f) * k;
    const bool derive = kids.derive[a] != 0;
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    uint32_t c[4];
    long long s[4], w[4];
    uint32_t tc = 0;
    long long ts = 0, tw = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t b = lane * B + u;
        const bool in = u < B && b < k;
        c[u] = in ? cnt[base + b] : 0u;
        s[u] = in ? (long long)sum[base + b] : 0ll;
        w[u] = in ? (long long)wsum[base + b] : 0ll;
        if (derive && in) {  // (this wave alone reads and writes the bins of (slot, f))
            c[u] -= cnt[obase + b];
            s[u] -= (long long)sum[obase + b];
            w[u] -= (long long)wsum[obase + b];
            cnt[base + b] = c[u];
            sum[base + b] = (unsigned long long)s[u];
            wsum[base + b] = (unsigned long long)w[u];
        }
        tc += c[u];
        ts += s[u];
        tw += w[u];
    }
    uint32_t ic = tc;
    long long is = ts, iw = tw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_up(ic, o);
        const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
        if ((int)lane >= o) {
            ic += oc;
            is += os;
            iw += ow;
        }
    }
    const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
    double vnode;  // the node's own output: what both sides are pulled toward
    (void)hist_reg_term(qtot, ldexp((double)wtot, -s_w), n, s_l, p, lo, hi, parent, has_parent, &vnode);
    uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
    long long rs = is - ts, rw = iw - tw;
    double bimp = 0.0;
    uint32_t bj = 0, bnl = 0, have = 0;
    long long bql = 0, bwl = 0;
    for (uint32_t u = 0; u < B; u++) {
        const uint32_t j = lane * B + u;
        rc += c[u];
        rs += s[u];
        rw += w[u];
        if (j >= ne) break;
        const uint32_t nl = rc, nr = n - rc;
        if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) continue;
        double imp;
        if (!hist_reg_candidate(nl, nr, rs, rw, qtot, wtot, s_l, s_w, p, lo, hi, vnode, sg, &imp)) continue;
        if (!have || imp >= bimp) {
            have = 1;
            bimp = imp;
            bj = j;
            bnl = nl;
            bql = rs;
            bwl = rw;
        }
    }
    // the last maximum over the lanes: larger importance, then the later edge
    double wimp = bimp;
    uint32_t wj = bj, whave = have;
    for (int o = 32; o > 0; o >>= 1) {
        const double oimp = __shfl_xor(wimp, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || oimp > wimp || (oimp == wimp && oj > wj))) {
            whave = 1;
            wimp = oimp;
            wj = oj;
        }
    }
    HistPickDev* out = rec + (size_t)a * F + f;
    if (!whave) {
        if (lane == 0) *out = HistPickDev{0.0, 0ll, qtot, 0ll, wtot, 0u, 0u, 0u, f};
    } else if (have && bj == wj) {
        *out = HistPickDev{bimp, bql, qtot, bwl, wtot, bj, bnl, 1u, f};
    }
}

// --- symmetric trees under lambda_l1 / max_delta_step: steps 1 to 3 and 6 (no parent, the whole line) ---

// the term of an integer pair at its own thresholded, capped output
__device__ __forceinline__ double hist_sym_reg_side(long long q, double h, int s_l, const HistRegDev& p) {
    double v;
    return hist_reg_term(q, h, 0u, s_l, p, -INFINITY, INFINITY, 0.0, false, &v);
}

// t_a of one candidate, as hist_sym_term<true>
__device__ __forceinline__ double hist_sym_reg_term(uint32_t nl, uint32_t n, long long ql, long long wl, long long qtot, long long wtot,
                                                    uint32_t min_leaf, int s_l, int s_w, const HistRegDev& p, double min_gain, double own,
                                                    bool* splits) {
    *splits = false;
    const uint32_t nr = n - nl;
    if (nl == 0 || nr == 0 || nl < min_leaf || nr < min_leaf) return own;
    const double hl = ldexp((double)wl, -s_w), hr = ldexp((double)(wtot - wl), -s_w);
    if (!(hl >= p.min_hess && hr >= p.min_hess && hl + p.l2 > 0.0 && hr + p.l2 > 0.0)) return own;
    const double imp = hist_sym_reg_side(ql, hl, s_l, p) + hist_sym_reg_side(qtot - ql, hr, s_l, p);
    if (!(imp - own > min_gain)) return own;
    *splits = true;
    return imp;
}

// grid F, 256 threads, as hist_scan_sym_kernel<true>
__global__ __launch_bounds__(256) void hist_scan_sym_reg_kernel(const HistItemDev* __restrict__ nodes, uint32_t A, uint32_t F, uint32_t k,
                                                                const uint32_t* __restrict__ nedges, const uint32_t* __restrict__ fsel,
                                                                const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                                const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                                HistRegDev p, double min_gain, HistSymBestDev* __restrict__ best) {
    __shared__ double tile[HIST_SYM_TILE][HIST_MAX_BINS];
    __shared__ uint8_t took[HIST_SYM_TILE][HIST_MAX_BINS];
    __shared__ double red_key[4];
    __shared__ uint32_t red_j[4], red_have[4];
    const uint32_t f = blockIdx.x, e = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t ne = min(nedges[fsel ? fsel[f] : f], k - 1);
    const uint32_t B = (k + 63) / 64;  // bins per lane (<= 4)
    double I = 0.0;
    uint32_t any = 0;
    for (uint32_t a0 = 0; a0 < A; a0 += HIST_SYM_TILE) {
        const uint32_t na = min(HIST_SYM_TILE, A - a0);
        for (uint32_t t = wave; t < na; t += 4) {  // (uniform in a wave: the shuffles below see all 64 lanes)
            const HistItemDev nd = nodes[a0 + t];
            const uint32_t n = nd.end - nd.begin;
            const size_t base = ((size_t)nd.slot * F + f) * k;
            uint32_t c[4];
            long long s[4], w[4];
            uint32_t tc = 0;
            long long ts = 0, tw = 0;
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t b = lane * B + u;
                const bool in = u < B && b < k;
                c[u] = in ? cnt[base + b] : 0u;
                s[u] = in ? (long long)sum[base + b] : 0ll;
                w[u] = in ? (long long)wsum[base + b] : 0ll;
                tc += c[u];
                ts += s[u];
                tw += w[u];
            }
            uint32_t ic = tc;
            long long is = ts, iw = tw;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t oc = __shfl_up(ic, o);
                const long long os = __shfl_up(is, o), ow = __shfl_up(iw, o);
                if ((int)lane >= o) {
                    ic += oc;
                    is += os;
                    iw += ow;
                }
            }
            const long long qtot = __shfl(is, 63), wtot = __shfl(iw, 63);
            const double own = hist_sym_reg_side(qtot, ldexp((double)wtot, -s_w), s_l, p);
            uint32_t rc = ic - tc;  // counts / sums of the bins before this lane's
            long long rs = is - ts, rw = iw - tw;
            for (uint32_t u = 0; u < B; u++) {
                const uint32_t j = lane * B + u;
                rc += c[u];
                rs += s[u];
                rw += w[u];
                if (j >= ne) break;  // (ne <= 255: j stays inside the tile's row)
                bool sp;
                tile[t][j] = hist_sym_reg_term(rc, n, rs, rw, qtot, wtot, min_leaf, s_l, s_w, p, min_gain, own, &sp);
                took[t][j] = sp ? 1 : 0;
            }
        }
        __syncthreads();
        if (e < ne) {
            for (uint32_t t = 0; t < na; t++) {  // node order: the sum's order is the definition's
                const double term = tile[t][e];
                I = (a0 + t == 0) ? term : I + term;
                any |= took[t][e];
            }
        }
        __syncthreads();
    }
    // the last maximum over the edges: larger key, then the later edge
    double wkey = (I != I) ? -INFINITY : I;
    uint32_t wj = e, whave = (e < ne && any) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        const double okey = __shfl_xor(wkey, o);
        const uint32_t oj = __shfl_xor(wj, o), ohave = __shfl_xor(whave, o);
        if (ohave && (!whave || okey > wkey || (okey == wkey && oj > wj))) {
            whave = 1;
            wkey = okey;
            wj = oj;
        }
    }
    if (lane == 0) {
        red_key[wave] = wkey;
        red_j[wave] = wj;
        red_have[wave] = whave;
    }
    __syncthreads();
    if (e == 0) {
        for (uint32_t v = 1; v < 4; v++) {
            if (red_have[v] && (!whave || red_key[v] > wkey || (red_key[v] == wkey && red_j[v] > wj))) {
                whave = 1;
                wkey = red_key[v];
                wj = red_j[v];
            }
        }
        best[f] = whave ? HistSymBestDev{wkey, wj, 1u} : HistSymBestDev{0.0, 0u, 0u};
    }
}

// grid A, one wave per open node, as hist_sym_apply_kernel<true>
__global__ __launch_bounds__(64) void hist_sym_apply_reg_kernel(const HistItemDev* __restrict__ nodes, uint32_t F, uint32_t k, uint32_t f, uint32_t j,
                                                                const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ sum,
                                                                const unsigned long long* __restrict__ wsum, uint32_t min_leaf, int s_l, int s_w,
                                                                HistRegDev p, double min_gain, HistBestNewtonDev* __restrict__ out) {
    const uint32_t a = blockIdx.x, lane = threadIdx.x;
    const HistItemDev nd = nodes[a];
    const uint32_t n = nd.end - nd.begin;
    const size_t base = ((size_t)nd.slot * F + f) * k;
    uint32_t nl = 0;
    long long ql = 0, wl = 0, qtot = 0, wtot = 0;
    for (uint32_t b = lane; b < k; b += 64) {
        const uint32_t c = cnt[base + b];
        const long long s = (long long)sum[base + b], w = (long long)wsum[base + b];
        qtot += s;
        wtot += w;
        if (b <= j) {
            nl += c;
            ql += s;
            wl += w;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {  // (integer sums: any order)
        nl += __shfl_xor(nl, o);
        ql += __shfl_xor(ql, o);
        wl += __shfl_xor(wl, o);
        qtot += __shfl_xor(qtot, o);
        wtot += __shfl_xor(wtot, o);
    }
    if (lane != 0) return;
    const double own = hist_sym_reg_side(qtot, ldexp((double)wtot, -s_w), s_l, p);
    bool sp;
    const double imp = hist_sym_reg_term(nl, n, ql, wl, qtot, wtot, min_leaf, s_l, s_w, p, min_gain, own, &sp);
    out[a] = HistBestNewtonDev{imp, ql, qtot, wl, wtot, j, nl, sp ? 1u : 0u, 0u};
}
