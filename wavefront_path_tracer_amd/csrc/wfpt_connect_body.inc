// The body of the connect kernels, included into connect_kernel, connect_power_kernel, connect_analytic_kernel, connect_shading_kernel and connect_nmap_kernel (wfpt_kernels.hip): one text, so that each kernel
// is compiled from its own statements and connect_kernel keeps its instructions whatever the other one gains (a shared function is optimised
// on its own first, and then schedules differently). In scope: the kernel's template parameters Trail, PRIM, LDS_SCENE, EXACT, TEX, ENVS and
// MIS, the constants POWER, ANALYTIC, SHADING and NMAP, the argument `a` (ConnectArgs), `ld` (LightDist; read where POWER is set only), `lt`
// (LightTable; read where ANALYTIC is set only), `sn` (the per-primitive normal rows; read where SHADING is set only) and `nm` (NmapScene;
// read where NMAP is set only).
    extern __shared__ float4 lds[];
    WFPT_SCENE_LDS(LDS_SCENE, s_stack); // (HBM-resident scenes: s_stack holds the walk's stack columns)
    const float4 *g_nodes = reinterpret_cast<const float4 *>(a.scene.nodes);
    const bool sampler = a.sample_in != nullptr;
    const uint32_t per_smp = sampler ? (a.sample_n + kChunk - 1u) / kChunk : a.n_chunks_max;
    const uint32_t n_items = sampler ? per_smp : per_smp * a.w.batch.n;
    const uint32_t frame0 = sampler ? 0u : uniform(a.w.ctl->frame.frame); // the batch's first frame, as shade_kernel and aov_body take it
    constexpr bool NO_EMITTERS = ENVS || ANALYTIC; // the kernels that run while no material emits (prim_em is null then)
    bool staged = false;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t smp = sampler ? 0u : item / per_smp, chunk = item - smp * per_smp;
        uint32_t count;
        if (sampler) {
            count = umin(static_cast<uint32_t>(kChunk), a.sample_n - chunk * kChunk);
        } else { // the segment's hits among those the step shades
            if (!segment_hits(a.w, sample_hits(a.w, smp), chunk, count)) continue;
            count = umin(count, static_cast<uint32_t>(kChunk));
        }
        count = uniform(count);
        if (count == 0u) continue;
        if (LDS_SCENE && !staged) {
            WFPT_STAGE_SCENE(g_nodes);
            __syncthreads();
            staged = true;
        }
        bool live = threadIdx.x < count;
        float3_ p = {0.0f, 0.0f, 0.0f}, n = p;
        float u0 = 0.0f, u1 = 0.0f, u2 = 0.0f;
        float u3 = 0.0f, u4 = 0.0f, share = 1.0f; // ENVS: the environment branch's two draws and the probability of the branch taken
        bool to_env = false;
        float4 *px = nullptr, *out = nullptr;
        float4 rec1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live && sampler) {
            const float *row = a.sample_in + (ENVS ? 10u : 9u) * (static_cast<size_t>(chunk) * kChunk + threadIdx.x);
            p = {row[0], row[1], row[2]};
            n = {row[3], row[4], row[5]};
            if (ENVS) {
                u1 = row[6]; u2 = row[7]; u3 = row[8]; u4 = row[9];
                to_env = true;
                if (MIS) share = a.envd.share;
            } else {
                u0 = row[6]; u1 = row[7]; u2 = row[8];
            }
        } else if (live) {
            // the hit's point, pixel and primitive: load_hit's two forms in this kernel's own statement order, with which three instantiations
            // at the SGPR ceiling keep their VGPR count (DESIGN.md 9k)
            const size_t slot = smp * static_cast<size_t>(a.w.batch.queue_stride) + static_cast<size_t>(chunk) * kChunk + threadIdx.x;
            uint32_t prim, pixel_idx;
            if (a.w.rec_in) {
                const float4 ra = a.w.rec_in[2u * slot], rb = a.w.rec_in[2u * slot + 1u];
                p = {ra.x, ra.y, ra.z};
                pixel_idx = __float_as_uint(ra.w);
                prim = __float_as_uint(rb.w);
            } else {
                const RayQueue q = slice(a.w.q, smp * static_cast<size_t>(a.w.batch.ray_stride));
                const float t = a.w.hq.t()[slot];
                const uint32_t ridx = a.w.hq.ridx()[slot];
                prim = a.w.hq.prim()[slot];
                p = {q.ox()[ridx] + t * q.dx()[ridx], q.oy()[ridx] + t * q.dy()[ridx], q.oz()[ridx] + t * q.dz()[ridx]}; // sh:91
                pixel_idx = q.pixel()[ridx];
            }
            const float4 rec0 = a.scene.shade_rec[3u * prim];
            rec1 = a.scene.shade_rec[3u * prim + 1u];
            const uint32_t m = material_class(a.scene.shade_rec, prim);
            if (a.w.material != 0xffffffffu && m != a.w.material) {
                live = false; // one per-material shade stage: its class only
            } else {
                const uint32_t lp = local_pixel(pixel_idx, a.w.image_width, a.w.tile);
                out = pixel_of(a.emitted + smp * static_cast<size_t>(a.w.batch.image_stride), lp);
                // (ENVS, ANALYTIC: no emission table while no material emits)
                if (m != 0u || ((!NO_EMITTERS || a.prim_em) && a.prim_em[prim] != kNoEmission)) { // metal, dielectric, emitter: the flag is cleared, nothing else
                    out->w = 0.0f;
                    live = false;
                } else {
                    px = pixel_of(a.w.image + smp * static_cast<size_t>(a.w.batch.image_stride), lp);
                    // the normal scatter() uses, never flipped
                    n = PRIM == 0 ? normalize3({p.x - rec0.x, p.y - rec0.y, p.z - rec0.z}) : float3_{rec0.x, rec0.y, rec0.z};
                    if (SHADING) shading_normal_at(a.scene.prim_geom, sn, prim, p, {rec0.x, rec0.y, rec0.z}, n); // (triangles: n is the stored normal here)
                    if (NMAP) mapped_normal_at(nm, a.scene.prim_geom, prim, p, {rec0.x, rec0.y, rec0.z}, n);
                    uint32_t rng = jenkins_hash(pixel_idx ^ jenkins_hash(frame0 + smp)); // init_rng((x, y), (W, H), frame): x + y W is the pixel
                    rng = jenkins_hash(rng ^ (0x9E3779B9u * (a.wavefront + 1u)));
                    u0 = rng_next_float(rng);
                    u1 = rng_next_float(rng);
                    u2 = rng_next_float(rng);
                    if (ENVS) { // the map with probability envd.share (the effective one: 1 with no light). At 1 there is no comparison:
                        // u0 = 1.0f must never reach an empty light list, nor a division by 1 - 1
                        to_env = !(a.envd.share < 1.0f) || u0 < a.envd.share;
                        if (to_env) {
                            share = a.envd.share;
                            u3 = rng_next_float(rng);
                            u4 = rng_next_float(rng);
                        } else {
                            share = 1.0f - a.envd.share;
                            u0 = (u0 - a.envd.share) / share;
                        }
                    }
                }
            }
        }
        LightSample s;
        bool lit = false, occluded = false;
        if (ENVS && to_env) lit = sample_env<MIS>(a.envd, n, u1, u2, u3, u4, share, s);
        else if (live) lit = sample_light<PRIM, TEX, MIS, POWER, ANALYTIC>(a, p, n, u0, u1, u2, s, ld, lt);
        if (lit) {
#if WFPT_STAMPS
            uint32_t dbg[3] = {0, 0, 0};
#endif
            // (the map: any hit occludes. Started with the closest-hit walk's own far end the early-out walk answers "is there a hit": kOccNone
            // means the reference tests no primitive below 1e30, kOccHit that it accepts one)
            float window = (ENVS && to_env) ? 1e30f : s.dist * 0.999f;
            if (ANALYTIC && is_sun(s)) window = 1e30f; // (a directional light's sample takes the map's window and rule)
            uint32_t verdict = kOccUndecided;
            // scenes in LDS, conservative boxes: the early-out walk answers most rays (DESIGN.md 9h: 3.4 % of a Shirley frame, same booleans)
            if (WFPT_NEE_EARLY_OUT && LDS_SCENE && !EXACT && !far_origin(a.scene, p.x, p.y, p.z))
                verdict = occluded_conservative<Trail, PRIM, uint16_t>(s_nodes, s_geom, s_parent, p.x, p.y, p.z, s.w.x, s.w.y, s.w.z,
                                                                      a.scene.n_nodes, window WFPT_DBG_ARG);
            if (verdict == kOccUndecided) { // every other scene kind, and the rays that walk hands back: the closest hit decides
                float t = 0.0f;
                uint32_t prim = 0;
                bool hit = false;
                WFPT_TRACE_ANY(g_nodes, s_stack, p.x, p.y, p.z, s.w.x, s.w.y, s.w.z);
                occluded = hit && ((ENVS && to_env) || t < window);
                if (ANALYTIC && is_sun(s)) occluded = hit;
            } else {
                occluded = verdict == kOccHit;
            }
        }
        if (ENVS && MIS && !to_env && lit) s.pl = s.pl * share; // plq: the light list's density times the share of the samples that go to it
        if (MIS && live && sampler) { // (q, primitive, (e_q G) wl, occluded, pl, pb, wl, 0): zeros where the sample contributes nothing
            float *row = a.sample_out + 12u * (static_cast<size_t>(chunk) * kChunk + threadIdx.x);
            float wl = lit ? s.pl / (s.pl + s.pb) : 0.0f; // (sample_light sets pl and pb only where it answers true)
            if (ANALYTIC && lit && is_analytic(s)) wl = 1.0f; // (the scatter never produces an analytic light's sample)
            if (ENVS) s.q = s.w; // (wdir, texel, (e Genv) we, occluded, pe, pb, we, 0)
            row[0] = s.q.x; row[1] = s.q.y; row[2] = s.q.z;
            row[3] = static_cast<float>(s.prim);
            if (ANALYTIC) row[3] = static_cast<float>(static_cast<int32_t>(s.prim)); // (analytic light j: -(1 + j))
            row[4] = lit ? (s.e.x * s.G) * wl : 0.0f; row[5] = lit ? (s.e.y * s.G) * wl : 0.0f; row[6] = lit ? (s.e.z * s.G) * wl : 0.0f;
            row[7] = occluded ? 1.0f : 0.0f;
            row[8] = lit ? s.pl : 0.0f; row[9] = lit ? s.pb : 0.0f; row[10] = wl; row[11] = 0.0f;
        } else if (MIS && live) {
            const float4 thr = *px, had = *out;
            const size_t lp4 = static_cast<size_t>(out - reinterpret_cast<float4 *>(a.emitted)); // the pixel's float4 in `emitted`: `origin` has its shape
            a.origin[lp4] = make_float4(p.x, p.y, p.z, 0.0f);
            if (ENVS && lit && !occluded && !to_env) { // an emitter of an ENVS context: the division by its share before the weight
                const float wl = s.pl / (s.pl + s.pb);
                *out = make_float4(had.x + ((((thr.x * rec1.x) * s.e.x) * s.G) / share) * wl, had.y + ((((thr.y * rec1.y) * s.e.y) * s.G) / share) * wl,
                                   had.z + ((((thr.z * rec1.z) * s.e.z) * s.G) / share) * wl, 1.0f);
            } else if (lit && !occluded) {
                float wl = s.pl / (s.pl + s.pb);
                if (ANALYTIC && is_analytic(s)) wl = 1.0f; // (an analytic light's sample is not weighed: x * 1 is x)
                *out = make_float4(had.x + (((thr.x * rec1.x) * s.e.x) * s.G) * wl, had.y + (((thr.y * rec1.y) * s.e.y) * s.G) * wl,
                                   had.z + (((thr.z * rec1.z) * s.e.z) * s.G) * wl, 1.0f);
            } else {
                out->w = 1.0f;
            }
        } else if (live && sampler) {
            float *row = a.sample_out + 8u * (static_cast<size_t>(chunk) * kChunk + threadIdx.x);
            if (ENVS) s.q = s.w;
            row[0] = s.q.x; row[1] = s.q.y; row[2] = s.q.z;
            row[3] = static_cast<float>(s.prim);
            if (ANALYTIC) row[3] = static_cast<float>(static_cast<int32_t>(s.prim)); // (analytic light j: -(1 + j))
            row[4] = lit ? s.e.x * s.G : 0.0f; row[5] = lit ? s.e.y * s.G : 0.0f; row[6] = lit ? s.e.z * s.G : 0.0f;
            row[7] = occluded ? 1.0f : 0.0f;
        } else if (live) {
            const float4 thr = *px, had = *out;
            if (ENVS && lit && !occluded && !to_env) // an emitter, picked with probability `share` = 1 - envd.share: the last operation
                *out = make_float4(had.x + (((thr.x * rec1.x) * s.e.x) * s.G) / share, had.y + (((thr.y * rec1.y) * s.e.y) * s.G) / share,
                                   had.z + (((thr.z * rec1.z) * s.e.z) * s.G) / share, 1.0f);
            else if (lit && !occluded)
                *out = make_float4(had.x + ((thr.x * rec1.x) * s.e.x) * s.G, had.y + ((thr.y * rec1.y) * s.e.y) * s.G,
                                   had.z + ((thr.z * rec1.z) * s.e.z) * s.G, 1.0f);
            else
                out->w = 1.0f;
        }
    }
