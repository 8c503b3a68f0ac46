// Host-side plan construction for the fused MLP (included by mlp.hip).
// Reference: noisy_src/model.py:83-221 (layer shapes, skip concat order
// [x_enc, h], colour input [feat, d_enc], parameter registration order).

namespace nr {

static int blocks_of(int n) { return (n + 31) / 32; }

bool make_plan(const NrMlpConfig* c, MlpPlan* p, const char** why) {
    std::memset(p, 0, sizeof(*p));
    if (!c) {
        *why = "null config";
        return false;
    }
    if (c->hidden != kHidden) {
        *why = "hidden_dim must be 256 (the MFMA tiling is specialised for it)";
        return false;
    }
    if (c->n_layers < 1 || c->n_layers > kMaxTrunk) {
        *why = "num_hidden_layers must be in [1, 16]";
        return false;
    }
    if (c->precision != NR_PREC_FP32 && c->precision != NR_PREC_BF16 && c->precision != NR_PREC_FP16) {
        *why = "precision must be NR_PREC_FP32, NR_PREC_BF16 or NR_PREC_FP16";
        return false;
    }
    if ((c->skip_mask >> (c->n_layers - 1)) != 0) {
        // model.py:125-126 sizes sigma/feature layers for `hidden` inputs, so a skip
        // after the last trunk layer is not a valid reference model either.
        *why = "skips must index trunk layers 0..num_hidden_layers-2";
        return false;
    }
    if (c->pos_freqs < 0 || c->dir_freqs < 0) {
        *why = "negative frequency count";
        return false;
    }
    p->L = c->pos_freqs;
    p->Ld = c->dir_freqs;
    p->n_layers = c->n_layers;
    p->skips = c->skip_mask;
    p->use_vd = c->use_view_dirs ? 1 : 0;
    p->prec = c->precision;
    p->dense_bwd = c->dense_backward ? 1 : 0;
    p->pos_dim = 3 * (1 + 2 * p->L);
    p->dir_dim = 3 * (1 + 2 * p->Ld);
    p->XB = blocks_of(p->pos_dim);
    p->DB = p->use_vd ? blocks_of(p->dir_dim) : 0;
    if (p->XB > 2 || blocks_of(p->dir_dim) > 1) {  // dir_freqs also when use_view_dirs is off: one envelope
        *why = "pos_freqs <= 10 and dir_freqs <= 4 are supported by the compiled kernels";
        return false;
    }
    const int n = p->n_layers;
    int64_t off = 0;
    auto set_lin = [&](LinearDesc& d, int out, int nseg, const Seg* segs) {
        d.out = out;
        d.in = 0;
        d.nseg = nseg;
        d.KB = 0;
        for (int s = 0; s < nseg; ++s) {
            d.seg[s] = segs[s];
            d.in += segs[s].width;
            d.KB += segs[s].blocks;
        }
        d.NB = blocks_of(out);
        d.w_off = off;
        off += static_cast<int64_t>(out) * d.in;
        d.b_off = off;
        off += out;
    };
    for (int i = 0; i < n; ++i) {
        Seg segs[2];
        int ns;
        if (i == 0) {
            segs[0] = {0, p->pos_dim, p->XB};
            ns = 1;
        } else if (is_skip(*p, i - 1)) {
            segs[0] = {0, p->pos_dim, p->XB};
            segs[1] = {p->pos_dim, kHidden, kHB};
            ns = 2;
        } else {
            segs[0] = {0, kHidden, kHB};
            ns = 1;
        }
        set_lin(p->lin[i], kHidden, ns, segs);
    }
    p->sig_w = off;  // sigma_linear (1, hidden)
    off += kHidden;
    p->sig_b = off;
    off += 1;
    {
        Seg s0[1] = {{0, kHidden, kHB}};
        set_lin(p->lin[n], kHidden, 1, s0);  // feature_linear
    }
    {
        Seg s1[2] = {{0, kHidden, kHB}, {kHidden, p->dir_dim, p->DB}};
        set_lin(p->lin[n + 1], kHidden / 2, p->use_vd ? 2 : 1, s1);  // dir_linear
    }
    p->rgb_w = off;  // rgb_linear (3, hidden/2)
    off += 3 * (kHidden / 2);
    p->rgb_b = off;
    off += 3;
    p->param_count = off;
    p->n_lin = n + 2;

    p->fpb = p->prec != NR_PREC_FP32 ? 2 : 4;
    // Forward images in forward stream order (trunk 0..n-1, feat, dir), then the
    // backward images in backward stream order (dir, feat, trunk n-1..0), so each
    // kernel's weight stream is one contiguous byte range.
    // 16-bit forward images are row-block major with each row block's bias
    // fragment appended (mlp_fwd_rbm.inc); fp32 ones chunk-major.
    int64_t pk = 0;
    for (int l = 0; l < p->n_lin; ++l) {
        LinearDesc& d = p->lin[l];
        d.pk_fwd = pk;
        const int bias_frag = p->fpb == 2 ? 1 : 0;
        pk += static_cast<int64_t>(d.NB) * (d.KB * p->fpb + bias_frag) * kFragBytes;
    }
    auto put_bwd = [&](int l) {
        LinearDesc& d = p->lin[l];
        d.pk_bwd = pk;
        pk += static_cast<int64_t>(d.NB) * d.KB * p->fpb * kFragBytes;
    };
    put_bwd(n + 1);
    put_bwd(n);
    for (int i = n - 1; i >= 0; --i) put_bwd(i);
    // 16-bit dX chain (mlp_bwd_rbm.inc): row-block-major W^T images of the hidden
    // input rows only (rows = the layer's h / feat input blocks, k = its outputs),
    // in stream order dir, feat, trunk n-1..1; a 256-wide stream per layer
    if (p->fpb == 2) {
        auto put_bwdr = [&](int l) {
            LinearDesc& d = p->lin[l];
            d.pk_bwdr = pk;
            pk += static_cast<int64_t>(kHB) * d.NB * 2 * kFragBytes;
        };
        put_bwdr(n + 1);
        put_bwdr(n);
        for (int i = n - 1; i >= 1; --i) put_bwdr(i);
    }
    // fp32 vectors in accumulator order [block][lane half][16 registers]:
    // each MFMA layer's bias, then w_sigma, then the 3 rows of W_rgb.
    for (int l = 0; l < p->n_lin; ++l) {
        p->lin[l].vb = pk;
        pk += static_cast<int64_t>(p->lin[l].NB) * 32 * 4;
    }
    p->vsig = pk;
    pk += kHidden * 4;
    p->vrgb = pk;
    pk += 3 * (kHidden / 2) * 4;
    p->vhead = pk;  // [w_sigma: kHB blocks][W_rgb row c: kHB/2 blocks] x (2 halves x 16 fp32), 3 whole KB
    pk += 3 * 1024;
    p->packed_bytes = pk;
    p->esize = p->prec != NR_PREC_FP32 ? 2 : 4;

    // saved tensors: xenc, h0..h_{n-1}, feat, denc, hc
    p->sv_F[SV_XENC] = p->XB * 32;
    for (int i = 0; i < n; ++i) p->sv_F[SV_H0 + i] = kHidden;
    p->sv_feat = n + 1;
    p->sv_denc = n + 2;
    p->sv_hc = n + 3;
    p->sv_F[p->sv_feat] = kHidden;
    p->sv_F[p->sv_denc] = p->DB * 32;
    p->sv_F[p->sv_hc] = kHidden / 2;
    p->n_saved = n + 4;
    p->n_mask = n + 1;
    // workspace dz tensors
    for (int i = 0; i < n; ++i) p->ws_F[WS_DZ0 + i] = kHidden;
    p->ws_feat = n;
    p->ws_dir = n + 1;
    p->ws_heads = n + 2;
    p->ws_F[p->ws_feat] = kHidden;
    p->ws_F[p->ws_dir] = kHidden / 2;
    p->ws_F[p->ws_heads] = 32;
    p->n_ws = n + 3;

    // dW jobs.  Layers are split by input tensor so that every tensor is staged
    // once: every trunk layer i > 0 has an h-job (dz_i x h_{i-1}); the x_enc
    // columns of layer 0 and of the skip layers share x-jobs ([dz_a, dz_b, ..] x
    // x_enc); the feature job also carries the sigma head ([dz_feat, dz_heads] x
    // h_{n-1}) and the dir job the rgb head ([dz_dir, dz_heads] x [feat, d_enc, h_c]),
    // so h_{n-1} is read once.
    int64_t slab = 0;
    int nj = 0, max_blk = 0;
    bool fits = true;
    // what the dW kernel assumes of every job, checked as the jobs and shares are made: grids
    // and shares inside dw_wave_pack's fields, a stage its waves can issue and LDS holds twice
    bool packs = true, stages = true;
    auto add_job = [&](int ndz, const DwSeg* dz, int nin, const DwSeg* in) {
        if (nj == kMaxJobs) {  // the caller's shares go to a scratch job; the plan fails
            fits = false;
            nj = kMaxJobs - 1;
        }
        DwJob& j = p->job[nj];
        j.ndz = ndz;
        j.nin = nin;
        j.NBz = 0;
        j.KB = 0;
        for (int s = 0; s < ndz; ++s) {
            j.dz[s] = dz[s];
            j.NBz += dz[s].blocks;
        }
        for (int s = 0; s < nin; ++s) {
            j.in[s] = in[s];
            j.KB += in[s].blocks;
        }
        packs = packs && j.NBz < 64 && j.KB < 64;
        stages = stages && (j.NBz + j.KB) * p->fpb <= dw_max_stage_pieces(p->fpb == 2);
        max_blk = j.NBz + j.KB > max_blk ? j.NBz + j.KB : max_blk;
        j.slab_off = slab;
        slab += static_cast<int64_t>(j.NBz) * 32 * (j.KB * 32 + 1);
        j.nwaves = 0;
        return nj++;
    };
    auto add_share = [&](DwJob& jb, const DwWave& sh) {
        if (jb.nwaves == kDwMaxWaves) {
            fits = false;
            return;
        }
        packs = packs && sh.np >= 1 && sh.np <= kDwMaxP && sh.nq >= 1 && sh.nq <= kDwMaxQ && sh.row0 >= 0 &&
                sh.row0 + sh.np <= jb.NBz && sh.col0 >= 0 && sh.col0 + sh.nq <= jb.KB;
        jb.w[jb.nwaves++] = sh;
    };
    // wave shares: rows [r0, r1) x cols [c0, c1) in 4 x 2 pieces, bias on the first column piece
    auto add_waves = [&](int j, int r0, int r1, int c0, int c1, bool bias) {
        for (int c = c0; c < c1; c += kDwMaxQ)
            for (int r = r0; r < r1; r += 4)
                add_share(p->job[j], {r, r1 - r < 4 ? r1 - r : 4, c, c1 - c < kDwMaxQ ? c1 - c : kDwMaxQ,
                                      bias && c == c0 ? 1 : 0});
    };
    int xjob[kMaxTrunk], xrow[kMaxTrunk], hjob[kMaxTrunk];
    {
        int layers[kMaxTrunk], nx = 0;
        for (int i = 0; i < n; ++i)
            if (i == 0 || is_skip(*p, i - 1)) layers[nx++] = i;
        // as many x-layers per job as its staged blocks allow: (cnt*kHB + XB) * FPB
        // pieces (dw_max_stage_pieces), and its shares 8 waves
        int per = kMaxJobSeg;
        while (per > 1 && ((per * kHB + p->XB) * p->fpb > dw_max_stage_pieces(p->fpb == 2) ||
                           per * (kHB / 4) * ((p->XB + kDwMaxQ - 1) / kDwMaxQ) > kDwMaxWaves))
            --per;
        for (int a = 0; a < nx; a += per) {
            DwSeg dz[kMaxJobSeg];
            const int cnt = nx - a < per ? nx - a : per;
            for (int b = 0; b < cnt; ++b) dz[b] = {1, WS_DZ0 + layers[a + b], kHB};
            DwSeg in[1] = {{0, SV_XENC, p->XB}};
            const int jb = add_job(cnt, dz, 1, in);
            add_waves(jb, 0, cnt * kHB, 0, p->XB, true);
            for (int b = 0; b < cnt; ++b) {
                xjob[layers[a + b]] = jb;
                xrow[layers[a + b]] = b * kHidden;
            }
        }
    }
    for (int i = 1; i < n; ++i) {
        DwSeg dz[1] = {{1, WS_DZ0 + i, kHB}};
        DwSeg in[1] = {{0, SV_H0 + i - 1, kHB}};
        hjob[i] = add_job(1, dz, 1, in);
        add_waves(hjob[i], 0, kHB, 0, kHB, true);
    }
    int jfeat, jdir, jsig = -1, sig_row = kHidden;
    if (p->fpb == 2) {
        // rows: dz_feat blocks 0..7, dz_heads block 8 (sigma); cols: h_{n-1}.  Waves
        // 4..7 take rows 4..8 (the 5-row shape); the heads block's bias comes from jdir
        DwSeg dz[2] = {{1, p->ws_feat, kHB}, {1, p->ws_heads, 1}};
        DwSeg in[1] = {{0, SV_H0 + n - 1, kHB}};
        jfeat = add_job(2, dz, 1, in);
        DwJob& jb = p->job[jfeat];
        for (int c = 0; c < kHB; c += kDwMaxQ) add_share(jb, {0, 4, c, kDwMaxQ, c == 0 ? 1 : 0});
        for (int c = 0; c < kHB; c += kDwMaxQ) add_share(jb, {4, kHB + 1 - 4, c, kDwMaxQ, c == 0 ? 1 : 0});
        jsig = jfeat;
    } else {
        // fp32 is MFMA-bound in dW, and a SIMD's two waves' blocks set its time: the
        // feature layer keeps 4 x 2 shares (16 blocks per SIMD, as an h-job) and the sigma
        // head ([dz_heads] x h_{n-1}, row 0 reduced) is a job of its own
        DwSeg dz[1] = {{1, p->ws_feat, kHB}};
        DwSeg in[1] = {{0, SV_H0 + n - 1, kHB}};
        jfeat = add_job(1, dz, 1, in);
        add_waves(jfeat, 0, kHB, 0, kHB, true);
        DwSeg dzh[1] = {{1, p->ws_heads, 1}};
        jsig = add_job(1, dzh, 1, in);
        add_waves(jsig, 0, 1, 0, kHB, false);
        sig_row = 0;
    }
    {
        // rows: dz_dir blocks 0..3, dz_heads block 4; cols: feat, [d_enc,] h_c
        const int DBu = p->use_vd ? p->DB : 0;
        DwSeg dz[2] = {{1, p->ws_dir, kHB / 2}, {1, p->ws_heads, 1}};
        DwSeg in[3] = {{0, p->sv_feat, kHB}, {0, p->sv_denc, p->DB}, {0, p->sv_hc, kHB / 2}};
        if (!p->use_vd) in[1] = in[2];
        jdir = add_job(2, dz, p->use_vd ? 3 : 2, in);
        add_waves(jdir, 0, kHB / 2, 0, kHB + DBu, true);               // dz_dir x [feat, d_enc]
        add_waves(jdir, kHB / 2, kHB / 2 + 1, kHB + DBu, kHB + DBu + kHB / 2, true);  // dz_heads x h_c
    }
    if (!fits) {
        // x-jobs hold two x_enc-reading layers each: n + ceil((skips + 1) / 2) <= 23 (fp32: 22)
        *why = "dW job shares exceed the 8-wave workgroup (too many skips for this depth: num_hidden_layers + "
               "ceil((len(skips) + 1) / 2) must not exceed 23, or 22 in fp32)";
        return false;
    }
    if (!packs) {
        *why = "a dW wave share lies outside its job's grid of at most 63 x 63 blocks";
        return false;
    }
    if (!stages) {
        *why = "a dW job stages more blocks per tile than its waves issue or LDS holds twice";
        return false;
    }
    p->dw_stage_bytes = max_blk * p->fpb * kFragBytes;
    // as many stages as fit beside the 1 KB of scratch: 4 for bf16, 2 for fp32
    p->dw_nstage = (kDwLdsBytes - kFragBytes) / p->dw_stage_bytes;
    if (p->dw_nstage > NR_DW_NSTAGE) p->dw_nstage = NR_DW_NSTAGE;
    int red = 0;
    auto add_red = [&](int rows, int in, int64_t w_off, int64_t b_off, int bjob, int brow0) -> ReduceRange& {
        ReduceRange& r = p->red[red++];
        r.rows = rows;
        r.in = in;
        r.w_off = w_off;
        r.b_off = b_off;
        r.nseg = 0;
        r.bjob = bjob;
        r.brow0 = brow0;
        return r;
    };
    auto add_seg = [](ReduceRange& r, int col0, int width, int job, int row0, int c0) {
        r.seg[r.nseg++] = {col0, width, job, row0, c0};
    };
    for (int i = 0; i < n; ++i) {
        const LinearDesc& d = p->lin[i];
        const bool has_x = i == 0 || is_skip(*p, i - 1);
        ReduceRange& r = add_red(kHidden, d.in, d.w_off, d.b_off, i > 0 ? hjob[i] : xjob[i], i > 0 ? 0 : xrow[i]);
        if (has_x) add_seg(r, 0, p->pos_dim, xjob[i], xrow[i], 0);
        if (i > 0) add_seg(r, has_x ? p->pos_dim : 0, kHidden, hjob[i], 0, 0);
    }
    {
        const LinearDesc& d = p->lin[n];
        add_seg(add_red(kHidden, kHidden, d.w_off, d.b_off, jfeat, 0), 0, kHidden, jfeat, 0, 0);
    }
    {
        // heads: dz_heads row 0 = sigma, rows 1..3 = rgb; biases from jdir's heads block
        const int hrow = kHidden / 2, hc_col = (kHB + (p->use_vd ? p->DB : 0)) * 32;
        add_seg(add_red(1, kHidden, p->sig_w, p->sig_b, jdir, hrow), 0, kHidden, jsig, sig_row, 0);
        add_seg(add_red(3, kHidden / 2, p->rgb_w, p->rgb_b, jdir, hrow + 1), 0, kHidden / 2, jdir, hrow + 1, hc_col);
    }
    {
        const LinearDesc& d = p->lin[n + 1];
        ReduceRange& r = add_red(kHidden / 2, d.in, d.w_off, d.b_off, jdir, 0);
        add_seg(r, 0, kHidden, jdir, 0, 0);
        if (p->use_vd) add_seg(r, kHidden, p->dir_dim, jdir, 0, kHidden);
    }
    p->n_jobs = nj;
    p->n_red = red;
    p->slab_floats_per_chunk = slab;
    if (p->prec != NR_PREC_FP32) return true;
    int slot;  // the chunk-major chains' weight streams, counted and not built
    return fwd_stream(*p, nullptr, &slot, why) && bwd_stream(*p, true, nullptr, &slot, why) &&
           bwd_stream(*p, false, nullptr, &slot, why);
}

static int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

MlpSizes make_sizes(const MlpPlan& p, int64_t M) {
    MlpSizes s;
    std::memset(&s, 0, sizeof(s));
    s.tiles = (M + 31) / 32;
    // whole 16-tile groups with at least one tile to spare: every fwd/bwd wave may store its
    // tile, and the last one is the dX chain's scratch tile (waves without an active tile)
    s.tiles_alloc = (s.tiles + 16) / 16 * 16 + kScratchTiles;
    int64_t off = 0;
    for (int t = 0; t < p.n_saved; ++t) {
        s.saved_off[t] = off;
        off = align256(off + s.tiles_alloc * p.sv_F[t] * 32 * p.esize);
    }
    s.mask_off = off;
    off = align256(off + s.tiles_alloc * p.n_mask * 64 * 16);
    s.saved_bytes = off;
    off = 0;
    for (int t = 0; t < p.n_ws; ++t) {
        s.ws_off[t] = off;
        off = align256(off + s.tiles_alloc * p.ws_F[t] * 32 * p.esize);
    }
    // dW: one round of workgroups (one per CU over the 256 CUs; same dW time as two
    // rounds, and half the chunk slabs for the reduction to read), at least 16 tiles
    // per chunk
#ifndef NR_DW_WGS
#define NR_DW_WGS 256
#endif
    int64_t ch = NR_DW_WGS / (p.n_jobs > 0 ? p.n_jobs : 1);
    if (ch > s.tiles / 16) ch = s.tiles / 16;
    s.chunks = static_cast<int>(ch < 1 ? 1 : ch);
    for (int j = 0; j < p.n_jobs; ++j) s.job_chunks[j] = s.chunks;
    s.max_chunks = s.chunks;
    if (p.fpb == 4 && p.n_jobs > 0) {
        // fp32 dW is MFMA-bound and every active wave runs the compiled 4 x 2 share, so a
        // job's time per tile is its busiest SIMD's: waves w and w + 4 share one (2 units
        // with more than 4 active waves, else 1).  One round of NR_DW_WGS workgroups is
        // dealt greedily to the job with the largest cost / workgroups (min-max), at
        // least 16 tiles per chunk; the uniform grid left the light jobs' CUs idle.
        int64_t cap = s.tiles / 16;
        if (cap < 1) cap = 1;
        int cost[kMaxJobs], left = NR_DW_WGS - p.n_jobs;
        for (int j = 0; j < p.n_jobs; ++j) {
            cost[j] = p.job[j].nwaves > kDwMaxWaves / 2 ? 2 : 1;
            s.job_chunks[j] = 1;
        }
        for (; left > 0; --left) {
            int best = -1;
            for (int j = 0; j < p.n_jobs; ++j) {
                if (s.job_chunks[j] >= cap) continue;
                // cost[j] / c[j] > cost[best] / c[best], in integers
                if (best < 0 || cost[j] * s.job_chunks[best] > cost[best] * s.job_chunks[j]) best = j;
            }
            if (best < 0) break;
            ++s.job_chunks[best];
        }
        s.max_chunks = 1;
        for (int j = 0; j < p.n_jobs; ++j) s.max_chunks = s.job_chunks[j] > s.max_chunks ? s.job_chunks[j] : s.max_chunks;
    }
    s.slab_off = off;
    off = align256(off + static_cast<int64_t>(s.max_chunks) * p.slab_floats_per_chunk * 4);
    // active tiles of the backward (tiles whose incoming gradient is not all zero): a
    // flag byte per tile of every segment of kSegTiles and the active count of each
    // 64-tile block (tile_flags_kernel), the dW kernel's list and its length
    s.nseg = (s.tiles + kSegTiles - 1) / kSegTiles;
    s.flags_off = off;
    off = align256(off + std::max<int64_t>(s.tiles_alloc, s.nseg * kSegTiles));
    s.blkcnt_off = off;
    off = align256(off + s.nseg * (kSegTiles / 64) * 4);
    s.dwlist_off = off;
    off = align256(off + s.tiles * 4);
    s.count_off = off;
    off = align256(off + 16);
    s.ws_bytes = off;
    return s;
}

FrozenSizes make_frozen_sizes(const MlpPlan& p, int64_t M) {
    FrozenSizes f;
    std::memset(&f, 0, sizeof(f));
    const MlpSizes t = make_sizes(p, M);
    f.tiles = t.tiles;
    f.nseg = t.nseg;
    if (p.fpb != 2) {
        // fp32: the training buffers (the chunk-major backward reads the activations)
        f.saved_bytes = t.saved_bytes;
        f.ws_bytes = t.ws_bytes;
        return f;
    }
    f.saved_bytes = f.tiles * p.n_mask * kFragBytes;
    f.scratch_base = f.tiles;
    const int64_t img_tiles = f.tiles + kScratchTiles;
    int64_t off = 0;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l > 0 && !is_skip(p, l - 1)) continue;
        f.keep_dz |= 1u << l;
        f.dz_off[l] = off;
        off = align256(off + img_tiles * kHidden * 32 * p.esize);
    }
    f.dz_dir_off = off;
    off = align256(off + img_tiles * (kHidden / 2) * 32 * p.esize);
    f.flags_off = off;
    off = align256(off + f.nseg * kSegTiles);
    f.blkcnt_off = off;
    off = align256(off + f.nseg * (kSegTiles / 64) * 4);
    f.ws_bytes = off;
    return f;
}

DinOffsets din_offsets(const MlpPlan& p, const MlpSizes& z) {
    DinOffsets o{};
    o.tiles = z.tiles;
    o.flags_off = z.flags_off;
    for (int l = 0; l < p.n_layers; ++l)
        if (l == 0 || is_skip(p, l - 1)) o.dz_off[l] = z.ws_off[WS_DZ0 + l];
    o.dz_dir_off = z.ws_off[p.ws_dir];
    return o;
}

DinOffsets din_offsets(const MlpPlan& p, const FrozenSizes& f) {
    DinOffsets o{};
    o.tiles = f.tiles;
    o.flags_off = f.flags_off;
    for (int l = 0; l < p.n_layers; ++l) o.dz_off[l] = f.dz_off[l];  // 0 outside keep_dz
    o.dz_dir_off = f.dz_dir_off;
    return o;
}

// ---------------------------------------------------------- launch descriptors ----
namespace {
// A weight stream in the making: its chunk count and largest load, and with `sd` its table
struct StreamFill {
    StreamDesc* sd;
    int nq, slot_kb;
    bool fits;

    // a layer's chunks behind the stream's, unless they pass kMaxChunks
    void push(int nchunks, int chunk_kb, int load_kb) {
        fits = fits && nq + nchunks <= kMaxChunks;
        if (!fits) return;
        for (int c = 0; sd && c < nchunks; ++c) {
            sd->ckb[nq + c] = load_kb;
            sd->cadv[nq + c] = chunk_kb;
        }
        nq += nchunks;
        slot_kb = load_kb > slot_kb ? load_kb : slot_kb;
    }

    bool close(int64_t base, int slot_max, int* slot_bytes, const char** why) {
        if (!fits) {
            *why = "an fp32 weight stream has more than kMaxChunks chunks";
            return false;
        }
        if (slot_kb * 1024 > slot_max) {
            *why = "a chunk of an fp32 weight stream exceeds its LDS slot";
            return false;
        }
        if (sd) {
            sd->base = base;
            sd->nq = nq;
        }
        *slot_bytes = slot_kb * 1024;
        return true;
    }
};
}  // namespace

bool fwd_stream(const MlpPlan& p, StreamDesc* sd, int* slot_bytes, const char** why) {
    StreamFill f{sd, 0, 0, true};
    for (int l = 0; l < p.n_lin; ++l) f.push(p.lin[l].KB, p.lin[l].NB * p.fpb, p.lin[l].NB * p.fpb);
    return f.close(p.lin[0].pk_fwd, kFwdSlotMax, slot_bytes, why);
}

bool bwd_stream(const MlpPlan& p, bool want_x, StreamDesc* sd, int* slot_bytes, const char** why) {
    const int n = p.n_layers;
    StreamFill f{sd, 0, 0, true};
    for (int l = n + 1; l >= (want_x ? 0 : 1); --l) {  // dir^T, feat^T, trunk n-1 .. 1 [, 0]
        const bool partial = !want_x && ((l > 0 && l < n && is_skip(p, l - 1)) || l == n + 1);
        f.push(p.lin[l].NB, p.lin[l].KB * p.fpb, partial ? kHB * p.fpb : p.lin[l].KB * p.fpb);
    }
    return f.close(p.lin[n + 1].pk_bwd, kBwdSlotMax, slot_bytes, why);
}

bool dw_args(const MlpPlan& p, const MlpSizes& z, const char* saved, char* workspace, DwArgs* w, int* nwg,
             size_t* lds, const char** why) {
    std::memset(w, 0, sizeof(*w));
    w->slabs = reinterpret_cast<float*>(workspace + z.slab_off);
    w->tiles = z.tiles;
    w->list = reinterpret_cast<const uint32_t*>(workspace + z.dwlist_off);
    w->count = reinterpret_cast<const uint32_t*>(workspace + z.count_off);
    w->njobs = p.n_jobs;
    *nwg = 0;
    for (int c = 0; c < z.max_chunks; ++c)
        for (int j = 0; j < p.n_jobs; ++j)
            if (c < z.job_chunks[j]) {
                if (*nwg == kDwMaxWgs) {
                    *why = "the dW chunks make more than kDwMaxWgs = 256 workgroups";
                    return false;
                }
                w->wg_map[(*nwg)++] = static_cast<uint16_t>(j | c << 5);
            }
    w->slab_floats_per_chunk = p.slab_floats_per_chunk;
    int min_chunks = z.job_chunks[0];
    for (int j = 0; j < p.n_jobs; ++j) {
        const DwJob& jb = p.job[j];
        w->job_chunks[j] = z.job_chunks[j];
        min_chunks = z.job_chunks[j] < min_chunks ? z.job_chunks[j] : min_chunks;
        w->job_NBz[j] = jb.NBz;
        w->job_KB[j] = jb.KB;
        w->job_slab[j] = jb.slab_off;
        for (int v = 0; v < jb.nwaves; ++v)  // the other waves idle: 0
            w->job_wave[j][v] = dw_wave_pack(jb.w[v].row0, jb.w[v].np, jb.w[v].col0, jb.w[v].nq, jb.w[v].bias);
        int ns = 0;
        auto add_seg = [&](const DwSeg& sg) {
            w->seg_ptr[j][ns] = sg.is_ws ? workspace + z.ws_off[sg.tensor] : saved + z.saved_off[sg.tensor];
            w->seg_blocks[j][ns++] = static_cast<uint8_t>(sg.blocks);
        };
        for (int q = 0; q < jb.ndz; ++q) add_seg(jb.dz[q]);
        for (int q = 0; q < jb.nin; ++q) add_seg(jb.in[q]);
    }
    w->stage_bytes = p.dw_stage_bytes;
    w->nstage = p.dw_nstage;
    *lds = static_cast<size_t>(w->nstage) * w->stage_bytes + kFragBytes;
    // the largest chunk's list entries behind the stages, when they fit
    const size_t list_bytes = (static_cast<size_t>((z.tiles + min_chunks - 1) / min_chunks) * 4 + 15) / 16 * 16;
    if (*lds + list_bytes <= static_cast<size_t>(kDwLdsBytes)) {
        w->list_lds = static_cast<int>(*lds);
        *lds += list_bytes;
    }
    if (*lds > static_cast<size_t>(kDwLdsBytes)) {
        *why = "the dW staging exceeds kDwLdsBytes = 160 KiB of LDS";
        return false;
    }
    return true;
}

int reduce_args(const MlpPlan& p, const MlpSizes& z, const char* workspace, float* g_params, ReduceArgs* r) {
    std::memset(r, 0, sizeof(*r));
    r->slabs = reinterpret_cast<const float*>(workspace + z.slab_off);
    r->g = g_params;
    r->inv_gscale = 1.0f / grad_scale(p.prec);
    r->param_count = p.param_count;
    r->slab_floats_per_chunk = p.slab_floats_per_chunk;
    r->n_red = p.n_red;
    int max_rows = 1;
    for (int k = 0; k < p.n_red; ++k) {
        const ReduceRange& rr = p.red[k];
        r->rows[k] = rr.rows;
        r->in[k] = rr.in;
        r->nseg[k] = rr.nseg;
        r->bjob[k] = rr.bjob;
        r->brow0[k] = rr.brow0;
        r->w_off[k] = rr.w_off;
        r->b_off[k] = rr.b_off;
        for (int q = 0; q < rr.nseg; ++q) r->seg[k][q] = rr.seg[q];
        max_rows = rr.rows > max_rows ? rr.rows : max_rows;
    }
    for (int j = 0; j < p.n_jobs; ++j) {
        r->job_slab[j] = p.job[j].slab_off;
        r->job_KB[j] = p.job[j].KB;
        r->job_chunks[j] = z.job_chunks[j];
    }
    return max_rows;
}

}  // namespace nr
