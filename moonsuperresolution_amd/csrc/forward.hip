// forward.hip — running the plan: launch_all, msr_forward / msr_forward_gated with the HIP-graph cache, and the per-family
// profiling entries.
#include "host.h"

using namespace msr;

enum Family { FAM_CONV = 0, FAM_SMALLCIN, FAM_MOMENTS, FAM_NORMACT, FAM_DENSE, FAM_LATENT, FAM_HEAD, FAM_DIRECT,
              FAM_COUNT };
static const char* kFamilyName[FAM_COUNT] = {"conv_igemm", "conv_smallcin", "moments", "norm_act", "dense",
                                             "latent", "head_up_conv4x4", "conv_direct"};

static hipEvent_t get_event(msr_handle* h) {
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        h->ev_pool.push_back(e);
    }
    return h->ev_pool[h->ev_used++];
}

// The launch plan of one generator(call): every kernel of msr_forward, on `s` and the handle's auxiliary stream.
static int launch_all(msr_handle* h, const float* in_dev, const float* eps_dev, float* out_dev, hipStream_t s,
                      hipEvent_t gate = nullptr) {
    // Fork: ops that need only the call's input go to the auxiliary stream.  With per-kernel profiling on they are
    // simply not timed (the brackets of the main-stream kernels stay valid: waits sit before the start event).
    const bool use_aux = h->aux != nullptr;
    if (use_aux) {
        bool any = false;
        for (auto& op : h->ops) any |= op.on_aux;
        if (any) {
            // Under stream capture the fork must hang off a real node of the call's stream: with the event record as the very
            // first captured operation the auxiliary branch becomes a second ROOT of the graph, and a replay was observed to
            // start that branch before earlier work of the launch stream had finished (a torch copy into the input buffer:
            // tests/test_gpu_generator.py::test_graph_replay_equals_eager, only after other processes had used the GPU).  A
            // 16-byte memset node in front of the fork makes the graph single-rooted.
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            if (s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive) {
                float* touch = D(h, "ws.aux_touch");
                if (touch) HIPCHK(h, hipMemsetAsync(touch, 0, 16, s));
            }
            HIPCHK(h, hipEventRecord(h->ev_fork, s));
            HIPCHK(h, hipStreamWaitEvent(h->aux, h->ev_fork, 0));
            for (auto& op : h->ops) {
                if (!op.on_aux) continue;
                SmallCinParams p = op.sc;
                p.src = in_dev;
                hipError_t e = launch_conv_smallcin(p, h->aux);
                if (e != hipSuccess) return fail(h, MSR_ERR_DEVICE, "launch of conv_smallcin (aux) failed: %s", hipGetErrorString(e));
                if (op.done) HIPCHK(h, hipEventRecord(op.done, h->aux));
            }
        }
    }
    // prof_on == 2: only the dominant family is timed, and a run of consecutive conv launches shares one pair of
    // events (an event costs the stream 2-3 us; bracketing all ~100 launches of a call costs 7 % of the throughput)
    ProfRec run{FAM_CONV, nullptr, nullptr, 0.0, 0.0, 0};
    auto close_run = [&]() {
        if (run.launches > 0) {
            run.b = get_event(h);
            hipEventRecord(run.b, s);
            h->prof.push_back(run);
        }
        run = ProfRec{FAM_CONV, nullptr, nullptr, 0.0, 0.0, 0};
    };
    int op_index = -1;
    for (auto& op : h->ops) {
        ++op_index;
        if (use_aux && op.on_aux) continue;
        if (gate && op_index == h->gate_op) {
            // msr_forward_gated: the matrix-bound part of this call starts only after the caller's event (the end of
            // the previous call on another handle / stream); everything before it overlaps that call's tail
            if (h->prof_on == 2) close_run();
            HIPCHK(h, hipStreamWaitEvent(s, gate, 0));
        }
        if (h->prof_on == 2 && ((op.type != OP_CONV && op.type != OP_GBR) || (use_aux && op.wait))) close_run();
        if (use_aux && op.wait) HIPCHK(h, hipStreamWaitEvent(s, op.wait, 0));
        hipEvent_t ea = nullptr, eb = nullptr;
        if (h->prof_on == 1) { ea = get_event(h); eb = get_event(h); hipEventRecord(ea, s); }
        if (h->prof_on == 2 && (op.type == OP_CONV || op.type == OP_GBR)) {
            if (run.launches == 0) { run.a = get_event(h); hipEventRecord(run.a, s); }
            run.launches += 1;
            run.flops += op.flops;
            run.bytes += op.bytes;
        }
        hipError_t e = hipSuccess;
        int fam = 0;
        switch (op.type) {
            case OP_CONV: {
                fam = FAM_CONV;
                ConvParams cp = op.conv;
                cp.partial = h->conv_partial;
                cp.mom_partial = h->mom_partial;
                cp.stat_partial = op.stat_slabs > 0 ? h->stat_ws : nullptr;
                e = launch_conv(cp, op.epi, op.kernel, op.tile, s);
                break;
            }
            case OP_SMALLCIN: {
                fam = FAM_SMALLCIN;
                SmallCinParams p = op.sc;
                if (op.src_is_input) p.src = in_dev;
                e = launch_conv_smallcin(p, s);
                break;
            }
            case OP_MOMENTS:
                fam = FAM_MOMENTS;
                e = launch_moments(op.mom.x, op.mom.G, op.mom.P, op.mom.C, op.mom.eps, h->mom_partial, op.mom.mean,
                                   op.mom.stdv, s);
                break;
            case OP_MOMENTS_SLABS:
                fam = FAM_MOMENTS;
                e = launch_moments_from_slabs(h->stat_ws, op.mom.P, op.mom.C, op.mom.eps, h->mom_partial, op.mom.mean,
                                              op.mom.stdv, s);
                break;
            case OP_NORMACT: fam = FAM_NORMACT; e = launch_norm_act(op.na, s); break;
            case OP_DENSE:
                fam = FAM_DENSE;
                e = launch_dense(op.dense.x, op.dense.W, op.dense.bias, h->dense_partial, op.dense.y, op.dense.B,
                                 op.dense.K, op.dense.N, s);
                break;
            case OP_LATENT:
                fam = FAM_LATENT;
                e = launch_latent(op.lat.mv, eps_dev, op.lat.z, op.lat.B, op.lat.L, op.lat.sampler, s);
                break;
            case OP_HEAD:
                fam = FAM_HEAD;
                e = launch_head(op.head.x, op.head.weff, op.head.bias, out_dev, op.head.B, op.head.r, op.head.C,
                                op.head.slope, op.head.tanh_out, op.head.x_py, op.head.x_pb, s);
                break;
            case OP_HEAD_GATHER:
                fam = FAM_HEAD;
                e = launch_head_gather(op.hg.partial, op.hg.bias, out_dev, op.hg.B, op.hg.r, s);
                break;
            case OP_GBR: {
                fam = FAM_CONV;
                GbrParams q = op.gbr;
                q.src = in_dev;
                e = launch_conv_gbr(q, op.gbr_ranges, s);
                break;
            }
            case OP_DIRECT: {
                fam = FAM_DIRECT;
                DirectConvParams p = op.dc;
                if (op.src_is_input) p.in0 = in_dev;
                if (op.out_is_output) p.out = out_dev;
                e = launch_conv_direct(p, s);
                break;
            }
        }
        if (e != hipSuccess)
            return fail(h, MSR_ERR_DEVICE, "launch of %s failed: %s", kFamilyName[fam], hipGetErrorString(e));
        if (h->prof_on == 1) { hipEventRecord(eb, s); h->prof.push_back({fam, ea, eb, op.flops, op.bytes, 1}); }
    }
    if (h->prof_on == 2) close_run();
    return MSR_OK;
}

extern "C" {

int msr_forward(msr_handle* h, const float* in_dev, const float* eps_dev, float* out_dev, int32_t batch,
                void* stream_v) {
    if (!h) return MSR_ERR_INVALID;
    if (!in_dev || !out_dev) return fail(h, MSR_ERR_INVALID, "msr_forward: null tensor pointer");
    if (batch != h->B)
        return fail(h, MSR_ERR_INVALID, "batch %d != batch_size %d the handle was created with "
                    "(the reference's sampler enforces the same, sampling.py:13-15)", batch, h->B);
    if (h->variant == MSR_GAUGAN && !eps_dev)
        return fail(h, MSR_ERR_INVALID, "variant gaugan needs the sampler noise eps [B, latent_dim]");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_plan(h);
    if (rc) return rc;
    h->forward_seen = true;
    hipStream_t s = (hipStream_t)stream_v;
    if (!h->graph_on || h->prof_on) return launch_all(h, in_dev, eps_dev, out_dev, s);
    // Graph mode: the ~100 launches, the fork to the auxiliary stream and its joins are captured once per pointer
    // triple and replayed with one hipGraphLaunch (the B = 1 latency case: the early kernels of a call are shorter
    // than a launch, and every cross-stream wait costs the stream ~16 us when issued eagerly).
    for (auto& g : h->graphs)
        if (g.in == in_dev && g.eps == eps_dev && g.out == out_dev) {
            g.last_use = ++h->graph_clock;
            HIPCHK(h, hipGraphLaunch(g.exec, s));
            return MSR_OK;
        }
    if (s == nullptr) return launch_all(h, in_dev, eps_dev, out_dev, s);     // the legacy default stream cannot be captured
    // A triple is captured on its second sighting: a caller that draws a fresh noise tensor (a fresh pointer) per call
    // never pays capture + instantiate, and never fills the cache with one-shot graphs.
    {
        bool seen = false;
        for (auto& t : h->seen_once) seen |= t.in == in_dev && t.eps == eps_dev && t.out == out_dev;
        if (!seen) {
            if (h->seen_once.size() >= 16) h->seen_once.erase(h->seen_once.begin());
            h->seen_once.push_back({in_dev, eps_dev, out_dev});
            return launch_all(h, in_dev, eps_dev, out_dev, s);
        }
    }
    if (h->graphs.size() >= 8) {                      // evict the least recently used graph (nothing of it may still run)
        size_t lru = 0;
        for (size_t k = 1; k < h->graphs.size(); ++k)
            if (h->graphs[k].last_use < h->graphs[lru].last_use) lru = k;
        HIPCHK(h, hipDeviceSynchronize());
        if (h->graphs[lru].exec) hipGraphExecDestroy(h->graphs[lru].exec);
        if (h->graphs[lru].graph) hipGraphDestroy(h->graphs[lru].graph);
        h->graphs.erase(h->graphs.begin() + lru);
    }
    msr_handle::GraphEntry e{in_dev, eps_dev, out_dev, nullptr, nullptr, ++h->graph_clock};
    HIPCHK(h, hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    rc = launch_all(h, in_dev, eps_dev, out_dev, s);
    hipError_t ce = hipStreamEndCapture(s, &e.graph);
    if (rc) { if (e.graph) hipGraphDestroy(e.graph); return rc; }
    if (ce != hipSuccess) return fail(h, MSR_ERR_DEVICE, "hipStreamEndCapture failed: %s", hipGetErrorString(ce));
    ce = hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0);
    if (ce != hipSuccess) {
        hipGraphDestroy(e.graph);
        return fail(h, MSR_ERR_DEVICE, "hipGraphInstantiate failed: %s", hipGetErrorString(ce));
    }
    h->graphs.push_back(e);
    HIPCHK(h, hipGraphLaunch(e.exec, s));
    return MSR_OK;
}

int msr_forward_gated(msr_handle* h, const float* in_dev, const float* eps_dev, float* out_dev, int32_t batch,
                      void* stream_v, void* gate_event) {
    if (!h) return MSR_ERR_INVALID;
    if (!gate_event) return msr_forward(h, in_dev, eps_dev, out_dev, batch, stream_v);
    if (!in_dev || !out_dev) return fail(h, MSR_ERR_INVALID, "msr_forward_gated: null tensor pointer");
    if (batch != h->B) return fail(h, MSR_ERR_INVALID, "batch %d != batch_size %d", batch, h->B);
    if (h->variant == MSR_GAUGAN && !eps_dev)
        return fail(h, MSR_ERR_INVALID, "variant gaugan needs the sampler noise eps [B, latent_dim]");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = ensure_plan(h);
    if (rc) return rc;
    h->forward_seen = true;
    return launch_all(h, in_dev, eps_dev, out_dev, (hipStream_t)stream_v, (hipEvent_t)gate_event);
}

int msr_graph_enable(msr_handle* h, int32_t on) {
    if (!h) return MSR_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->graph_on = on ? 1 : 0;
    if (!on) { HIPCHK(h, hipDeviceSynchronize()); drop_graphs(h); }
    return MSR_OK;
}

int msr_last_latent(msr_handle* h, float* z_dev, void* stream) {
    if (!h || !z_dev) return MSR_ERR_INVALID;
    if (!h->z) return fail(h, MSR_ERR_STATE, "no latent: run msr_forward on a SPADE variant first");
    HIPCHK(h, hipMemcpyAsync(z_dev, h->z, (size_t)h->B * h->L * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MSR_OK;
}

int msr_forward_flops(const msr_handle* hc, double* flops) {
    msr_handle* h = const_cast<msr_handle*>(hc);
    if (!h || !flops) return MSR_ERR_INVALID;
    int rc = ensure_plan(h);
    if (rc) return rc;
    *flops = h->fwd_flops;
    return MSR_OK;
}

int msr_profile_enable(msr_handle* h, int32_t on) {
    if (!h) return MSR_ERR_INVALID;
    if (on < 0 || on > 2) return fail(h, MSR_ERR_INVALID, "msr_profile_enable: mode must be 0, 1 or 2");
    h->prof_on = on;
    return MSR_OK;
}

int msr_profile_reset(msr_handle* h) {
    if (!h) return MSR_ERR_INVALID;
    hipDeviceSynchronize();
    h->prof.clear();
    h->ev_used = 0;
    return MSR_OK;
}

int msr_profile_read(msr_handle* h, msr_kernel_stat* out, int32_t cap, int32_t* n) {
    if (!h || !out || !n) return MSR_ERR_INVALID;
    HIPCHK(h, hipDeviceSynchronize());
    msr_kernel_stat st[FAM_COUNT];
    std::memset(st, 0, sizeof st);
    for (int f = 0; f < FAM_COUNT; ++f)
        std::snprintf(st[f].name, sizeof st[f].name, "%s%s", kFamilyName[f],
                      f == FAM_CONV ? (h->prec == PREC_BF16X3 ? "_bf16x3" : "_f32") : "");
    for (auto& r : h->prof) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, r.a, r.b));
        st[r.fam].launches += r.launches;
        st[r.fam].device_ms += ms;
        st[r.fam].flops += r.flops;
        st[r.fam].bytes += r.bytes;
    }
    int k = 0;
    for (int f = 0; f < FAM_COUNT && k < cap; ++f)
        if (st[f].launches) out[k++] = st[f];
    *n = k;
    return MSR_OK;
}

int msr_profile_runs(msr_handle* h, void* ref_event, int32_t family, double* start_ms, double* end_ms, double* flops,
                     int64_t* launches, int32_t cap, int32_t* n) {
    if (!h || !ref_event || !start_ms || !end_ms || !flops || !launches || !n || family < 0 || family >= FAM_COUNT)
        return MSR_ERR_INVALID;
    HIPCHK(h, hipDeviceSynchronize());
    int k = 0;
    for (auto& r : h->prof) {
        if (r.fam != family) continue;
        if (k >= cap) return fail(h, MSR_ERR_INVALID, "msr_profile_runs: %d records do not fit", (int)h->prof.size());
        float a = 0.f, b = 0.f;
        HIPCHK(h, hipEventElapsedTime(&a, (hipEvent_t)ref_event, r.a));
        HIPCHK(h, hipEventElapsedTime(&b, (hipEvent_t)ref_event, r.b));
        start_ms[k] = a; end_ms[k] = b; flops[k] = r.flops; launches[k] = r.launches;
        ++k;
    }
    *n = k;
    return MSR_OK;
}

}  // extern "C"
