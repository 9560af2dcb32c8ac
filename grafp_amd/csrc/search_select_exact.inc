// search_select_exact.inc -- the body of knn_search.hip's search_select_exact_kernel<TIGHTEN> and
// search_select_exact_half_kernel, included inside each (see the comment in front of them there).  It uses the kernel's
// parameters (db: const float * or const unsigned short *, the element type exact_l2 is overloaded on) and TIGHTEN.
    __shared__ float pend_d[4][WT_PEND];
    __shared__ int pend_i[4][WT_PEND];
    __shared__ float wtop_d[4][32];
    __shared__ int wtop_i[4][32];
    __shared__ float sq[SR_D];
    __shared__ float s_thr2;
    __shared__ int need_rows[SR_CAP];                      // every listed candidate fits: no overflow case
    __shared__ int s_nneed;
    const int qi = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < SR_D) sq[tid] = q[(size_t)qi * SR_D + tid];
    __shared__ int s_off[SR_NSUB + 1];
    const float myqq = qq[qi];
    if (wave == 0) {                                       // sub-list fills -> offsets of a flat candidate index
        const int cs = lane < SR_NSUB ? cnt[qi * SR_NSUB + lane] : 0;      // (one load per lane, a 16-lane prefix sum)
        const bool over = cs > SR_SUBCAP;
        const int v = over ? SR_SUBCAP : cs;
        int inc = v;
#pragma unroll
        for (int j = 1; j < SR_NSUB; j <<= 1) {
            const int o = __shfl_up(inc, j);
            if (lane >= j) inc += o;
        }
        const bool any_over = __ballot(over) != 0;
        if (lane < SR_NSUB) s_off[lane] = inc - v;
        if (lane == SR_NSUB - 1) s_off[SR_NSUB] = any_over ? -1 : inc;
    }
    __syncthreads();
    const int c = s_off[SR_NSUB];
    const bool listed = c >= 0;                            // else: a sub-list overflowed -> exact rescan of every row
    auto slot_of = [&](int e) {                            // flat candidate index -> slot in the query's list
        int s2 = 0;
#pragma unroll
        for (int b2 = SR_NSUB / 2; b2 > 0; b2 >>= 1) s2 += (e >= s_off[s2 + b2]) ? b2 : 0;
        return s2 * SR_SUBCAP + (e - s_off[s2]);
    };
    float thr2 = thr[qi];
    const float kminus = 1.0f - SB_SLACK, kplus = 1.0f + SB_SLACK;
    const float qhi = myqq * kplus, qlo = myqq * kminus, dspan = kplus - kminus;     // (kplus - kminus is exact)
    // ---- the pieces both selection methods are built from (one copy each) ----
    auto cand = [&](int e, int &row, float &ev, float &ddv) {    // flat index -> the scan's record (row, E, norm);
        const size_t sl = (size_t)qi * SR_CAP + slot_of(e < c ? e : c - 1);    // past the end: the last candidate,
        row = cand_i[sl];                                        // loaded instead of branched around
        const float2 ed = cand_e[sl];
        ev = ed.x;
        ddv = ed.y;                                              // the row's norm rides with the candidate: no gather
    };
    auto hi_of = [&](float ev, float ddv) {
        const float hi = __builtin_fmaf(dspan, ddv, __builtin_fmaf(-2.0f, ev, qhi));
        return hi < 0.0f ? 0.0f : hi;
    };
    auto keep = [&](bool valid, float ev, int row) {             // compaction: the rows with lo <= bound (no dd[row] needed)
        if (valid && __builtin_fmaf(-2.0f, ev, qlo) <= thr2) need_rows[atomicAdd(&s_nneed, 1)] = row;
    };
    WaveTop top;
    float td;
    int ti;
    // Phase A, the k-th smallest upper bound (or a bound on it), by one of two methods chosen from the list's size; each
    // ends with the compaction of the rows phase B has to look at.
    //   c <= SF_CAP (the usual case: a few hundred candidates): no sorting networks at all (a 64-lane bitonic sort is
    //   ~1 700 cycles, and the fold + three-sort merge of the other method ran twice per query: 16 of the kernel's 29 us
    //   at 41 queries, tools' stop-point timing, round 4).  The candidates (row, E, hi) stay in registers (up to eight
    //   per thread); the bound is read from a 256-bin histogram of hi between its minimum and maximum -- the upper edge
    //   (plus one bin against the rounding of the bin index) of the bin the k-th smallest falls into: >= the k-th
    //   smallest hi, so still a valid bound, a bin or two looser.
    //   Otherwise: WaveTop + merge, the exact k-th smallest hi.
    constexpr int SF_CAP = 2048, SF_NEED = 512, SF_PER = SF_CAP / 256;
    __shared__ int f_row[SF_NEED];
    __shared__ float f_hi[SF_NEED];
    __shared__ int f_hist[256];
    __shared__ float f_red[2][4];
    if (tid == 0) s_nneed = 0;                             // (both methods pass a barrier before they compact)
    if (listed && c <= SF_CAP) {
        int row[SF_PER];
        float ev[SF_PER], ddv[SF_PER], hi[SF_PER];
#pragma unroll
        for (int u = 0; u < SF_PER; ++u) {                 // every load of a kind in flight at once; the rounds past the
            row[u] = 0;                                    // end of the list (u * 256 >= c: uniform) load nothing
            ev[u] = 0.0f;
            ddv[u] = 0.0f;
            if (u * 256 < c) cand(u * 256 + tid, row[u], ev[u], ddv[u]);
        }
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < SF_PER; ++u) {
            hi[u] = hi_of(ev[u], ddv[u]);
            if (u * 256 + tid < c) {
                mn = fminf(mn, hi[u]);
                mx = fmaxf(mx, hi[u]);
            }
        }
        f_hist[tid] = 0;
#pragma unroll
        for (int j = 1; j < 64; j <<= 1) {
            mn = fminf(mn, __shfl_xor(mn, j));
            mx = fmaxf(mx, __shfl_xor(mx, j));
        }
        if (lane == 0) {
            f_red[0][wave] = mn;
            f_red[1][wave] = mx;
        }
        __syncthreads();
        const float lo_h = fminf(fminf(f_red[0][0], f_red[0][1]), fminf(f_red[0][2], f_red[0][3]));
        const float hi_h = fmaxf(fmaxf(f_red[1][0], f_red[1][1]), fmaxf(f_red[1][2], f_red[1][3]));
        const float w = (hi_h - lo_h) * (1.0f / 256.0f);
        const float inv = (w > 0.0f && w < INFINITY) ? 1.0f / w : 0.0f;
#pragma unroll
        for (int u = 0; u < SF_PER; ++u) {
            if (u * 256 + tid < c) {
                int b = (int)((hi[u] - lo_h) * inv);
                b = b < 0 ? 0 : (b > 255 ? 255 : b);
                atomicAdd(&f_hist[b], 1);
            }
        }
        __syncthreads();
        if (wave == 0) {                                   // bins 4 lane .. 4 lane + 3: inclusive scan over the lanes
            const int h0 = f_hist[4 * lane], h1 = f_hist[4 * lane + 1], h2 = f_hist[4 * lane + 2], h3 = f_hist[4 * lane + 3];
            const int mine = h0 + h1 + h2 + h3;
            int cum = mine;
#pragma unroll
            for (int j = 1; j < 64; j <<= 1) {
                const int o = __shfl_up(cum, j);
                if (lane >= j) cum += o;
            }
            const int before = cum - mine;                 // candidates in the bins of the lanes below
            if (c < k) {
                if (lane == 0) s_thr2 = INFINITY;          // fewer than k candidates exist
            } else if (before < k && cum >= k) {           // exactly one lane
                int b = 4 * lane, run = before + h0;
                if (run < k) { ++b; run += h1; }
                if (run < k) { ++b; run += h2; }
                if (run < k) { ++b; }
                s_thr2 = fminf(hi_h, __builtin_fmaf((float)(b + 2), w, lo_h));
            }
        }
        __syncthreads();
        thr2 = fminf(thr2, s_thr2);
        if (!TIGHTEN) {
#pragma unroll
            for (int u = 0; u < SF_PER; ++u) keep(u * 256 + tid < c, ev[u], row[u]);
        }
    } else if (listed) {
        top.init(pend_d[wave], pend_i[wave], INFINITY);
        // four candidates per thread and round, every load of a kind in flight at once: a list of 3 000 costs three
        // dependent round trips, not twelve
        for (int e0 = 0; e0 < c; e0 += 4 * 256) {
            int row[4];
            float ev[4], ddv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cand(e0 + u * 256 + tid, row[u], ev[u], ddv[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * 256 < c)                      // uniform: push is a wave-level call
                    top.push(e0 + u * 256 + tid < c, hi_of(ev[u], ddv[u]), row[u], k, lane);
        }
        if (top.pc > 0) top.fold(k, lane);
        block_merge_tops(top, wtop_d, wtop_i, wave, lane, td, ti);
        if (wave == 0 && lane == k - 1) s_thr2 = td;      // +inf when fewer than k candidates exist
        __syncthreads();
        thr2 = fminf(thr2, s_thr2);
        if (!TIGHTEN) {
            for (int e0 = 0; e0 < c; e0 += 4 * 256) {
                int row[4];
                float ev[4], ddv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) cand(e0 + u * 256 + tid, row[u], ev[u], ddv[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) keep(e0 + u * 256 + tid < c, ev[u], row[u]);
            }
        }
    }
    if (TIGHTEN) {
        if (tid == 0 && listed) thr[qi] = thr2;
        return;
    }
    __syncthreads();                                       // need_rows and its count stand; the merge buffers are free again
    const int nneed = listed ? s_nneed : 0;
    // Phase B, the exact distances (contract (1)-(2)) of the rows still in question -- compacted first and fetched one
    // per thread side by side: picked out of the candidate rounds where they stand, every round paid a full row-fetch
    // latency for its two or three scattered lanes -- and the k best of them, again by one of two methods.
    //   nneed <= SF_NEED (the usual hundred rows): every thread finds the RANK of its row by counting the (distance, id)
    //   pairs before it -- ranks < k are the answer, written in place.  O(need^2 / 256) compares per thread: 40 at the
    //   usual hundred rows.
    //   Otherwise, and for a query whose lists overflowed (every row of the database): WaveTop + merge.
    if (listed && nneed <= SF_NEED) {                      // (uniform)
        float dmine[SF_NEED / 256];
        int rmine[SF_NEED / 256];
#pragma unroll
        for (int v = 0; v < SF_NEED / 256; ++v) {
            const int i = v * 256 + tid;
            rmine[v] = i < nneed ? need_rows[i] : 0;
            dmine[v] = (v * 256 < nneed) ? (i < nneed ? exact_l2(db, dd, rmine[v], sq, myqq) : INFINITY) : INFINITY;
            if (i < nneed) {
                f_hi[i] = dmine[v];
                f_row[i] = rmine[v];
            }
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < SF_NEED / 256; ++v) {
            const int i = v * 256 + tid;
            if (v * 256 < nneed) {                         // uniform
                int rank = 0;
                for (int j = 0; j < nneed; ++j) rank += lex_lt(f_hi[j], f_row[j], dmine[v], rmine[v]) ? 1 : 0;
                if (i < nneed && rank < k) {
                    out_d[(size_t)qi * k + rank] = dmine[v];
                    out_i[(size_t)qi * k + rank] = id_base + (int64_t)rmine[v];
                }
            }
        }
        if (tid >= nneed && tid < k) {                     // fewer rows than k (k <= 32 < 256): contract (4)
            out_d[(size_t)qi * k + tid] = INFINITY;
            out_i[(size_t)qi * k + tid] = -1;
        }
        return;
    }
    top.init(pend_d[wave], pend_i[wave], thr2);
    const int64_t nrows = listed ? nneed : n;
    for (int64_t i0 = 0; i0 < nrows; i0 += 256) {
        const bool need = i0 + tid < nrows;
        const int64_t row = listed ? (need ? need_rows[i0 + tid] : 0) : i0 + tid;
        top.push(need, need ? exact_l2(db, dd, row, sq, myqq) : INFINITY, (int)row, k, lane);
    }
    if (top.pc > 0) top.fold(k, lane);
    block_merge_tops(top, wtop_d, wtop_i, wave, lane, td, ti);
    if (wave == 0 && lane < k) {
        out_d[(size_t)qi * k + lane] = td;
        out_i[(size_t)qi * k + lane] = ti == SR_EMPTY ? (int64_t)-1 : id_base + (int64_t)ti;
    }
