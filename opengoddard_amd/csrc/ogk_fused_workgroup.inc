// ogk_fused_workgroup.inc -- one workgroup of the one-launch form (ogk_kernels.hip includes this text into the body of
// ogk_fused and of ogk_fused_batch).  Expects in scope: `a` (const ogk_args&: the launch's argument block, or a lane's
// record), ndef, n_eval, group_lo, n_light, sum_lo, n_sum and the workgroup's LDS window `lds`.  Text, not a function:
// ogk_fused compiles to exactly what it was before batches existed.  The maintainable form - a __device__
// __forceinline__ function taking `const ogk_args&` - was tried first: ogk_fused then came out with other register
// numbers in one region (same instructions otherwise) and the module's slowest part took 0.13 - 0.15 s longer to
// compile in both of two alternating cold-start measurements (the inliner clones the launch's largest body), which
// is what a user who never batches would have paid.
    int id = (int)blockIdx.x;
    if (id < n_eval) {
        FZ_TRACE_DECL(0);
        if (!(OGK_FZ & 16)) {
            if (id < ndef) eval_defect_body<true>(a, id, lds);
            else eval_rows_body<true>(a, id - ndef, lds);
        }
        FZ_STAMP(1);
        finish_eval(a, (unsigned)n_eval, reinterpret_cast<unsigned*>(lds));
        FZ_STAMP(4);
        FZ_TRACE_OUT(a);
        return;
    }
    id -= n_eval;
    // nothing in the sweep workgroups waits for the evaluation workgroups (finish_eval).  Grid order (OGK_ORDER,
    // timing experiments): 0 = light, heavy parts, MFMA tiles; 1 = MFMA tiles, heavy parts, light; 2 = tiles and
    // light workgroups interleaved, heavy parts first
#ifndef OGK_ORDER
#define OGK_ORDER 0
#endif
    const int n_tile = OGT_N_FTILES, n_heavy = OGT_N_HPART;
    int kind, idx;                                     // 0 light, 1 heavy, 2 tile
    if (OGK_ORDER == 0) {
        if (id < n_light) kind = 0, idx = id;
        else if (id < n_light + n_heavy) kind = 1, idx = id - n_light;
        else kind = 2, idx = id - n_light - n_heavy;
    } else if (OGK_ORDER == 1) {
        if (id < n_tile) kind = 2, idx = id;
        else if (id < n_tile + n_heavy) kind = 1, idx = id - n_tile;
        else kind = 0, idx = id - n_tile - n_heavy;
    } else {
        if (id < n_heavy) kind = 1, idx = id;
        else {
            const int r = id - n_heavy, pairs = n_light < n_tile ? n_light : n_tile;
            if (r < 2 * pairs) kind = (r & 1) ? 0 : 2, idx = r >> 1;
            else if (n_light > n_tile) kind = 0, idx = r - pairs;
            else kind = 2, idx = r - pairs;
        }
    }
    // light workgroups: the ones that carry a sequential sum first (OGT_LSUM / OGT_LPLAIN: both in column order;
    // sum_lo of the first list and group_lo - sum_lo of the second lie below this launch's column range)
    // (n_sum < 0: column order - the launch fits one round of residency and the order only decides who shares a compute unit)
    if (kind == 0)
        fz_light_body(a, n_sum < 0 ? group_lo + idx
                                   : idx < n_sum ? OGT_LSUM[sum_lo + idx] : OGT_LPLAIN[group_lo - sum_lo + idx - n_sum], lds);
    else if (kind == 1) { if (!(OGK_FZ & 32)) fz_heavy_part(a, idx, lds); }
    else fz_tile_body(a, idx, lds);
