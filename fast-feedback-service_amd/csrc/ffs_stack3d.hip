// ffs_stack3d.hip -- rotation sweeps: the per-frame strong-pixel lists never leave the GPU; they are appended to the
// stack's device buffers and ffs_stack3d_finish labels the whole stack in 3D (kernels_stack3d.hpp).  Where a batch's lists land, the
// tables and launch sizes of the finish and which records are reflections are decided in sweep_plan.hpp; the lists of a batch on
// another context travel through ffs_multi.hip (multi_move_packed).
// Reference: ConnectedComponents::find_3d_components, spotfinder/connected_components/connected_components.cc:270-470;
// the driver's rotation_slices map, spotfinder/spotfinder.cc:913-918,1099-1148.
#include "ffs_internal.hpp"
#include "kernels_stack3d.hpp"

// Growable device (or pinned host) buffer of the 3D stack: reallocated with slack when too small
template <typename T>
struct PoolBuf {
    T* p = nullptr;
    size_t cap = 0;
    bool pinned_host = false;
    hipError_t ensure(size_t n, bool keep = false, hipStream_t st = nullptr) {
        if (n <= cap) return hipSuccess;
        const size_t want = pool_growth(n);
        T* q = nullptr;
        hipError_t e = pinned_host ? hipHostMalloc(reinterpret_cast<void**>(&q), want * sizeof(T), hipHostMallocDefault)
                                   : hipMalloc(reinterpret_cast<void**>(&q), want * sizeof(T) + 256);
        if (e != hipSuccess) return e;
        if (keep && p && cap) {
            e = hipMemcpyAsync(q, p, cap * sizeof(T), pinned_host ? hipMemcpyHostToHost : hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) { pinned_host ? (void)hipHostFree(q) : (void)hipFree(q); return e; }
        }
        release();
        p = q;
        cap = want;
        return hipSuccess;
    }
    void release() {
        if (p) pinned_host ? (void)hipHostFree(p) : (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct ffs_stack3d {
    ffs_ctx* ctx = nullptr;
    uint64_t max_total = 0;    // as given to ffs_stack3d_create (stack_has_room reads it)
    hipStream_t st = nullptr;  // the stack's own stream
    std::mutex mu;             // worker threads add their batches concurrently (the reference's rotation_slices_mutex)
    // slices as they arrive: lists appended to the arrival buffers on the device
    std::map<int64_t, HeldSlice> slices;  // frame id -> place in the arrival buffers (std::map order = z order, spotfinder.cc:1105-1108)
    uint64_t arrived = 0;
    PoolBuf<uint32_t> a_k, a_i;
    PoolBuf<StackSlice> d_table, h_table;
    // ffs_stack3d_add_batch does not wait for its append: each call takes the next of kSlots slice tables and leaves an
    // event behind; a slot is reused only after its event, and finish / a growing buffer / destroy wait for all of them
    static constexpr int kSlots = 8;
    PoolBuf<StackSlice> d_ring, h_ring;   // kSlots tables of ring_stride entries
    size_t ring_stride = 0;
    hipEvent_t slot_ev[kSlots] = {};
    bool slot_used[kSlots] = {};
    uint64_t n_adds = 0;
    // the stack in (z, k) order and the scratch of its labelling (sized in finish, kept for the next one)
    PoolBuf<uint32_t> d_k, d_i, d_z, d_parent, d_comp, d_begin, d_chunk_roots, d_small, d_sx, d_sy, d_sc;
    PoolBuf<CompAcc> d_acc;
    PoolBuf<ReflOut> d_recs;
    std::vector<ffs_reflection> out;
    // per-signal view of the last finish (vertex order)
    std::vector<uint32_t> sig_x, sig_y, sig_i;
    std::vector<int32_t> sig_z, sig_refl;
    float last_finish_ms = 0;
};

// the appends still in flight (ffs_stack3d_add_batch leaves them running) are done when this returns
static void stack3d_join_appends(ffs_stack3d* st) {
    for (int k = 0; k < ffs_stack3d::kSlots; ++k)
        if (st->slot_used[k]) {
            (void)hipEventSynchronize(st->slot_ev[k]);
            st->slot_used[k] = false;
        }
}

// what the last finish handed out
static void stack3d_clear_results(ffs_stack3d* st) {
    st->out.clear();
    st->sig_x.clear(); st->sig_y.clear(); st->sig_z.clear(); st->sig_i.clear(); st->sig_refl.clear();
}

// ---- 3D stack ------------------------------------------------------------------------------------------

static int stack3d_create_impl(ffs_ctx* c, uint64_t max_total, ffs_stack3d** out) {
    {   // a stack of this context that was destroyed: its stream and its (grown) buffers are ready -- a sweep's worth of
        // hipMalloc / hipFree is 1.5 ms, more than its 100 frames take on the GPU
        std::lock_guard<std::mutex> lock(c->stream_mu);
        if (!c->stack_pool.empty()) {
            ffs_stack3d* st = c->stack_pool.back();
            c->stack_pool.pop_back();
            st->max_total = max_total;
            *out = st;
            return FFS_OK;
        }
    }
    ffs_stack3d* st = new (std::nothrow) ffs_stack3d();
    if (!st) return FFS_ERR_NOMEM;
    st->ctx = c;
    st->max_total = max_total;
    st->h_table.pinned_host = true;
    HIP_TRY(c, hipSetDevice(c->device));
    hipError_t e = hipStreamCreateWithFlags(&st->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
        c->err = std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e);
        delete st;
        return FFS_ERR_DEVICE;
    }
    *out = st;
    return FFS_OK;
}

std::atomic<int> g_live_stacks{0};   // while one is alive, batches leave their strong-pixel lists on the device (tuning "device_lists" = 2)

extern "C" int ffs_stack3d_create(ffs_ctx* c, uint64_t max_total, ffs_stack3d** out) {
    if (!c || !out) return FFS_ERR_INVALID;
    *out = nullptr;
    const int rc = stack3d_create_impl(c, max_total, out);
    if (rc != FFS_OK) return rc;
    g_live_stacks.fetch_add(1);
    {
        std::lock_guard<std::mutex> lock(c->stream_mu);
        c->live_stacks.push_back(*out);
    }
    handle_add(kHandleStack, *out);
    return FFS_OK;
}

extern "C" void ffs_stack3d_destroy(ffs_stack3d* st) {
    if (!st || !handle_take(kHandleStack, st)) return;   // (destroyed already -- by its context's ffs_ctx_destroy, or twice)
    g_live_stacks.fetch_sub(1);
    ffs_ctx* c = st->ctx;   // alive: a context takes its stacks with it, and this one was still in the registry
    (void)hipSetDevice(c->device);
    {
        std::lock_guard<std::mutex> lock(c->stream_mu);
        auto& v = c->live_stacks;
        v.erase(std::remove(v.begin(), v.end(), st), v.end());
        if (c->stack_pool.size() < 2) {   // keep it, emptied, for the next sweep
            stack3d_join_appends(st);
            if (st->st) (void)hipStreamSynchronize(st->st);
            st->slices.clear();
            st->arrived = 0;
            st->n_adds = 0;
            stack3d_clear_results(st);
            st->last_finish_ms = 0;
            c->stack_pool.push_back(st);
            return;
        }
    }
    stack3d_free(st);
}

void stack3d_free(ffs_stack3d* st) {
    (void)hipSetDevice(st->ctx->device);
    stack3d_join_appends(st);
    for (int k = 0; k < ffs_stack3d::kSlots; ++k)
        if (st->slot_ev[k]) (void)hipEventDestroy(st->slot_ev[k]);
    if (st->st) (void)hipStreamSynchronize(st->st);
    st->d_ring.release(); st->h_ring.release();
    st->a_k.release(); st->a_i.release(); st->d_table.release(); st->h_table.release();
    st->d_k.release(); st->d_i.release(); st->d_z.release(); st->d_parent.release(); st->d_comp.release();
    st->d_begin.release(); st->d_chunk_roots.release(); st->d_small.release();
    st->d_sx.release(); st->d_sy.release(); st->d_sc.release(); st->d_acc.release(); st->d_recs.release();
    if (st->st) (void)hipStreamDestroy(st->st);
    delete st;
}

// room for `more` entries behind the ones that have arrived (the lists already there are kept)
static int stack3d_reserve(ffs_stack3d* st, uint64_t more) {
    ffs_ctx* c = st->ctx;
    if (!stack_has_room(st->arrived, more, st->max_total)) {
        c->err = "ffs_stack3d: too many strong pixels in the stack";
        return FFS_ERR_OVERFLOW;
    }
    if (st->arrived + more > st->a_k.cap || st->arrived + more > st->a_i.cap) stack3d_join_appends(st);  // (the buffers move)
    STK_TRY(c, st->a_k.ensure(st->arrived + more, true, st->st));
    STK_TRY(c, st->a_i.ensure(st->arrived + more, true, st->st));
    return FFS_OK;
}

static int stack3d_add_slice_impl(ffs_stack3d* st, int64_t frame_id, const uint32_t* k, const uint32_t* inten, uint32_t n) {
    ffs_ctx* c = st->ctx;
    std::lock_guard<std::mutex> lock(st->mu);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = stack3d_reserve(st, n);
    if (rc != FFS_OK) return rc;
    if (n) {
        STK_TRY(c, hipMemcpyAsync(st->a_k.p + st->arrived, k, (size_t)n * 4, hipMemcpyHostToDevice, st->st));
        STK_TRY(c, hipMemcpyAsync(st->a_i.p + st->arrived, inten, (size_t)n * 4, hipMemcpyHostToDevice, st->st));
        STK_TRY(c, hipStreamSynchronize(st->st));  // the caller's arrays may go away
    }
    st->slices[frame_id] = HeldSlice{(uint32_t)st->arrived, n};  // (a frame added twice: the later list counts)
    st->arrived += n;
    return FFS_OK;
}

extern "C" int ffs_stack3d_add_slice(ffs_stack3d* st, int64_t frame_id, const uint32_t* k,
                                     const uint32_t* inten, uint32_t n) {
    if (!st || (n && (!k || !inten))) return FFS_ERR_INVALID;
    return guarded(st->ctx, [&] { return stack3d_add_slice_impl(st, frame_id, k, inten, n); });
}

// ---- a batch's lists into the stack -----------------------------------------------------------------------------------------------------

// The placement's table goes up (h_tab -> d_tab) and k_stack_append copies the stream's device lists by it, both in the stream's sparse stream:
// behind the launch that wrote the lists, ahead of the one that will overwrite them
static int stack3d_launch_append(ffs_ctx* c, ffs_stream* s, const BatchPlacement& p, StackSlice* h_tab, StackSlice* d_tab, uint32_t* dst_k,
                                 uint32_t* dst_i) {
    const uint32_t nf = (uint32_t)p.table.size();
    std::memcpy(h_tab, p.table.data(), (size_t)nf * sizeof(StackSlice));
    STK_TRY(c, hipMemcpyAsync(d_tab, h_tab, (size_t)nf * sizeof(StackSlice), hipMemcpyHostToDevice, s->st2));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_stack_append, dim3(list_copy_blocks(p.biggest), nf), dim3(256), 0, s->st2, s->d_list_k, s->d_list_i, (uint64_t)s->cap,
                       d_tab, dst_k, dst_i);
    STK_TRY(c, hipGetLastError());
    return FFS_OK;
}

// the batch's frames are held where the placement put them (a frame added twice: the later list counts)
static void stack3d_hold(ffs_stack3d* st, const ffs_stream* s, const BatchPlacement& p) {
    for (uint32_t f = 0; f < s->n_frames; ++f)
        st->slices[s->results[f].frame_id] = HeldSlice{(uint32_t)p.dst[f], s->results[f].num_strong_pixels};
}

// Lists of a batch processed on ANOTHER context (same detector geometry, usually another GPU) into this stack: packed end
// to end on the source device, then one transfer per array.  Frames that overflowed the stream's lists were re-run on the
// stream's one-frame stream and have their lists on the host (as for a local batch): those go up from there.  Caller holds st->mu.
static int stack3d_add_batch_remote(ffs_stack3d* st, ffs_stream* s, const BatchPlacement& p) {
    ffs_ctx* c = st->ctx;       // home
    HIP_TRY(c, hipSetDevice(s->ctx->device));
    if (!s->d_pack_k) {
        const size_t cap_all = (size_t)s->max_batch * s->cap;
        if (dmalloc(&s->d_pack_k, cap_all * 4) != hipSuccess || dmalloc(&s->d_pack_i, cap_all * 4) != hipSuccess
            || dmalloc(&s->d_pack_tab, (size_t)s->max_batch * sizeof(StackSlice)) != hipSuccess
            || hipHostMalloc(reinterpret_cast<void**>(&s->h_pack_tab), (size_t)s->max_batch * sizeof(StackSlice), hipHostMallocDefault) != hipSuccess
            || hipEventCreateWithFlags(&s->ev_pack, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            c->err = "allocation of the list pack buffers failed";
            return FFS_ERR_NOMEM;
        }
    }
    if (p.packed == 0) return FFS_OK;
    // the pack buffers are free again once the previous batch's transfer out of them has completed (peer copies run in the
    // home stream; RCCL sends in this very stream)
    if (s->sent_pending) {
        STK_TRY(c, hipStreamWaitEvent(s->st2, s->ev_sent, 0));
        s->sent_pending = false;
    }
    FFS_TRY(stack3d_launch_append(c, s, p, s->h_pack_tab, s->d_pack_tab, s->d_pack_k, s->d_pack_i));
    return multi_move_packed(s, c, st->st, st->a_k.p + st->arrived, st->a_i.p + st->arrived, p.packed);
}

// The lists of the stream's last batch go from its device buffers to the stack's, device to device.
static int stack3d_add_batch_impl(ffs_stack3d* st, ffs_stream* s) {
    ffs_ctx* c = s->ctx;
    if (s->busy || s->results.empty()) {
        c->err = "ffs_stack3d_add_batch: call after ffs_wait()";
        return FFS_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lock(st->mu);
    const uint32_t nf = s->n_frames;
    std::vector<BatchFrame> frames(nf);
    uint64_t more = 0;
    for (uint32_t f = 0; f < nf; ++f) {
        frames[f] = BatchFrame{s->results[f].num_strong_pixels, overflow_frame(&s->ovf, f) != nullptr};
        more += frames[f].n;
    }
    for (uint32_t f = 0; f < nf; ++f) {
        // a frame that did not fit the stream's lists was re-run on its one-frame stream: its list is on the host, if kept
        if (frames[f].overflow && frames[f].n && overflow_frame(&s->ovf, f)->k.size() != frames[f].n) {
            c->err = "ffs_stack3d_add_batch: a frame overflowed the stream's lists; set want_strong_list (or a larger "
                     "max_strong_per_frame) for rotation sweeps";
            return FFS_ERR_OVERFLOW;
        }
    }
    ffs_ctx* home = st->ctx;
    const bool remote = s->ctx != st->ctx;
    if (remote && (home->L.W != c->L.W || home->L.H != c->L.H)) {
        c->err = "ffs_stack3d_add_batch: the stream's context has another frame shape than the stack's";
        return FFS_ERR_INVALID;
    }
    HIP_TRY(home, hipSetDevice(home->device));
    int rc = stack3d_reserve(st, more);
    if (rc != FFS_OK) { if (remote) c->err = home->err; return rc; }
    // where every frame's entries land (sweep_plan.hpp); overflow frames go up from the host, the others from the stream's device lists
    const BatchPlacement p = place_batch(st->arrived, frames, remote);
    hipStream_t up_st = remote ? st->st : s->st2;   // (remote: the stack's stream on the home device)
    for (uint32_t f = 0; f < nf; ++f) {
        if (!frames[f].overflow || !frames[f].n) continue;
        const OverflowFrame* o = overflow_frame(&s->ovf, f);
        STK_TRY(c, hipMemcpyAsync(st->a_k.p + p.dst[f], o->k.data(), (size_t)frames[f].n * 4, hipMemcpyHostToDevice, up_st));
        STK_TRY(c, hipMemcpyAsync(st->a_i.p + p.dst[f], o->inten.data(), (size_t)frames[f].n * 4, hipMemcpyHostToDevice, up_st));
    }
    if (remote) {
        rc = stack3d_add_batch_remote(st, s, p);
        if (rc != FFS_OK) { c->err = home->err; return rc; }
        if (p.host_lists) {   // (the overflow frames' lists live in the stream's result vectors)
            HIP_TRY(home, hipSetDevice(home->device));
            STK_TRY(c, hipStreamSynchronize(st->st));
        }
        stack3d_hold(st, s, p);
        st->arrived = p.end;
        (void)hipSetDevice(c->device);
        return FFS_OK;
    }
    // Local: the append runs in the stream's own sparse stream -- nothing to wait for here.  Its slice table sits in one of kSlots slots.
    const int slot = (int)(st->n_adds++ % ffs_stack3d::kSlots);
    if (st->ring_stride < c->max_batch || !st->d_ring.p) {
        stack3d_join_appends(st);
        st->ring_stride = std::max<size_t>(c->max_batch, nf);
        st->h_ring.pinned_host = true;
        STK_TRY(c, st->h_ring.ensure(st->ring_stride * ffs_stack3d::kSlots));
        STK_TRY(c, st->d_ring.ensure(st->ring_stride * ffs_stack3d::kSlots));
    }
    if (nf > st->ring_stride) {
        c->err = "ffs_stack3d_add_batch: batch larger than the context's max_batch";
        return FFS_ERR_INVALID;
    }
    if (!st->slot_ev[slot]) STK_TRY(c, hipEventCreateWithFlags(&st->slot_ev[slot], hipEventDisableTiming));
    if (st->slot_used[slot]) {
        STK_TRY(c, hipEventSynchronize(st->slot_ev[slot]));
        st->slot_used[slot] = false;
    }
    stack3d_hold(st, s, p);
    if (p.biggest)
        FFS_TRY(stack3d_launch_append(c, s, p, st->h_ring.p + (size_t)slot * st->ring_stride, st->d_ring.p + (size_t)slot * st->ring_stride,
                                      st->a_k.p, st->a_i.p));
    STK_TRY(c, hipEventRecord(st->slot_ev[slot], s->st2));
    st->slot_used[slot] = true;
    if (p.host_lists) STK_TRY(c, hipStreamSynchronize(s->st2));  // (the overflow frames' lists live in the stream's result vectors)
    st->arrived = p.end;
    return FFS_OK;
}

extern "C" int ffs_stack3d_add_batch(ffs_stack3d* st, ffs_stream* s) {
    if (!st || !s) return FFS_ERR_INVALID;
    if (!s->lists_valid) {   // (the stack was created after the batch was submitted, or tuning "device_lists" is 0)
        s->ctx->err = "ffs_stack3d_add_batch: this batch did not leave its strong-pixel lists on the device -- create the stack before "
                      "submitting (tuning \"device_lists\" 2) or set \"device_lists\" to 1";
        return FFS_ERR_INVALID;
    }
    return guarded(s->ctx, [&] { return stack3d_add_batch_impl(st, s); });
}

extern "C" int ffs_stack3d_signals(ffs_stack3d* st, const uint32_t** x, const uint32_t** y, const int32_t** z,
                                   const uint32_t** intensity, const int32_t** reflection, uint64_t* n) {
    if (!st) return FFS_ERR_INVALID;
    if (x) *x = st->sig_x.data();
    if (y) *y = st->sig_y.data();
    if (z) *z = st->sig_z.data();
    if (intensity) *intensity = st->sig_i.data();
    if (reflection) *reflection = st->sig_refl.data();
    if (n) *n = st->sig_refl.size();
    return FFS_OK;
}

// ---- finish: the held slices into (z, k) order, labelled as one segment --------------------------------------------------------------------

// the buffers of a finish over `plan`, its tables uploaded and its five kernels launched in the stack's stream; -> the components found
static int stack3d_label(ffs_stack3d* st, const FinishPlan& plan, uint32_t* n_calc) {
    ffs_ctx* c = st->ctx;
    const uint32_t N = (uint32_t)plan.total;
    const size_t nz = plan.table.size();
    STK_TRY(c, st->h_table.ensure(nz));
    STK_TRY(c, st->d_table.ensure(nz));
    STK_TRY(c, st->d_begin.ensure(nz + 1));
    STK_TRY(c, st->d_k.ensure(N)); STK_TRY(c, st->d_i.ensure(N)); STK_TRY(c, st->d_z.ensure(N));
    STK_TRY(c, st->d_parent.ensure(N)); STK_TRY(c, st->d_comp.ensure(N));
    STK_TRY(c, st->d_acc.ensure(N)); STK_TRY(c, st->d_recs.ensure(N));
    STK_TRY(c, st->d_chunk_roots.ensure(plan.chunks));
    STK_TRY(c, st->d_small.ensure(16));  // [0] n, [1] n_comp, [2] status, [8..15] summary
    STK_TRY(c, st->d_sx.ensure(N)); STK_TRY(c, st->d_sy.ensure(N)); STK_TRY(c, st->d_sc.ensure(N));
    std::memcpy(st->h_table.p, plan.table.data(), nz * sizeof(StackSlice));
    hipEvent_t e0, e1;
    STK_TRY(c, hipEventCreate(&e0));
    STK_TRY(c, hipEventCreate(&e1));
    const uint32_t small[16] = {N, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipEventRecord(e0, st->st);
    STK_TRY(c, hipMemcpyAsync(st->d_table.p, st->h_table.p, nz * sizeof(StackSlice), hipMemcpyHostToDevice, st->st));
    STK_TRY(c, hipMemcpyAsync(st->d_begin.p, plan.begin.data(), (nz + 1) * 4, hipMemcpyHostToDevice, st->st));
    STK_TRY(c, hipMemcpyAsync(st->d_small.p, small, sizeof(small), hipMemcpyHostToDevice, st->st));
    SegArgs sa{};
    sa.list_k = st->d_k.p;
    sa.list_i = st->d_i.p;
    sa.parent = st->d_parent.p;
    sa.comp_id = st->d_comp.p;
    sa.seg_n = st->d_small.p;
    sa.seg_stride = N;
    sa.n_comp = st->d_small.p + 1;
    sa.acc = st->d_acc.p;
    sa.max_comp = N;
    sa.overflow = st->d_small.p + 2;
    sa.W = (uint32_t)c->L.W;
    sa.H = (uint32_t)c->L.H;
    sa.row_off = nullptr;
    sa.slice_begin = st->d_begin.p;
    sa.n_slices = (int)nz;
    sa.zs = st->d_z.p;
    sa.min_spot_size = c->settings.params.min_spot_size_3d;
    sa.max_sep = c->settings.params.max_peak_centroid_separation;
    sa.recs = st->d_recs.p;
    sa.summary = st->d_small.p + 8;
    sa.chunk_roots = st->d_chunk_roots.p;
    sa.chunks_max = plan.chunks;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_stack_gather, dim3(plan.gather_blocks, (unsigned)nz), dim3(256), 0, st->st,
                       st->a_k.p, st->a_i.p, st->d_table.p, st->d_k.p, st->d_i.p, st->d_z.p, st->d_parent.p, st->d_acc.p);
    hipLaunchKernelGGL(k_union<true>, dim3(plan.entry_blocks, 1), dim3(256), 0, st->st, sa);
    hipLaunchKernelGGL(k_reduce_roots3d, dim3(plan.reduce_blocks), dim3(256), 0, st->st, sa);
    hipLaunchKernelGGL(k_finalize_roots3d, dim3(plan.finalize_blocks), dim3(256), 0, st->st, sa);
    hipLaunchKernelGGL(k_stack_labels, dim3(plan.entry_blocks), dim3(256), 0, st->st, sa, st->d_sx.p, st->d_sy.p, st->d_sc.p);
    STK_TRY(c, hipGetLastError());
    uint32_t back[16];
    STK_TRY(c, hipMemcpyAsync(back, st->d_small.p, sizeof(back), hipMemcpyDeviceToHost, st->st));
    (void)hipEventRecord(e1, st->st);
    STK_TRY(c, hipStreamSynchronize(st->st));
    (void)hipEventElapsedTime(&st->last_finish_ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *n_calc = back[1];
    return FFS_OK;
}

static int stack3d_finish_impl(ffs_stack3d* st, const ffs_reflection** reflections, uint32_t* n_refl,
                               uint32_t* n_calculated, uint32_t* n_f_size, uint32_t* n_f_sep) {
    ffs_ctx* c = st->ctx;
    std::lock_guard<std::mutex> lock(st->mu);
    HIP_TRY(c, hipSetDevice(c->device));
    for (int k = 0; k < ffs_stack3d::kSlots; ++k)   // the appends of the last batches may still be running (in other streams)
        if (st->slot_used[k]) HIP_TRY(c, hipStreamWaitEvent(st->st, st->slot_ev[k], 0));
    // z = rank of the frame id among the slices held (std::map order, spotfinder.cc:1105-1108)
    std::vector<HeldSlice> held;
    held.reserve(st->slices.size());
    for (const auto& kv : st->slices) held.push_back(kv.second);
    const FinishPlan plan = plan_finish(held, (uint32_t)kRootChunk);
    stack3d_clear_results(st);
    uint32_t n_calc = 0;
    RecordClasses classes;
    if (plan.total > 0) {
        const uint32_t N = (uint32_t)plan.total;
        FFS_TRY(stack3d_label(st, plan, &n_calc));
        std::vector<ReflOut> recs(n_calc);
        if (n_calc) STK_TRY(c, hipMemcpyAsync(recs.data(), st->d_recs.p, (size_t)n_calc * sizeof(ReflOut), hipMemcpyDeviceToHost, st->st));
        std::vector<uint32_t> comp(N), zs(N);
        st->sig_x.resize(N); st->sig_y.resize(N); st->sig_i.resize(N);
        STK_TRY(c, hipMemcpyAsync(st->sig_x.data(), st->d_sx.p, (size_t)N * 4, hipMemcpyDeviceToHost, st->st));
        STK_TRY(c, hipMemcpyAsync(st->sig_y.data(), st->d_sy.p, (size_t)N * 4, hipMemcpyDeviceToHost, st->st));
        STK_TRY(c, hipMemcpyAsync(st->sig_i.data(), st->d_i.p, (size_t)N * 4, hipMemcpyDeviceToHost, st->st));
        STK_TRY(c, hipMemcpyAsync(comp.data(), st->d_sc.p, (size_t)N * 4, hipMemcpyDeviceToHost, st->st));
        STK_TRY(c, hipMemcpyAsync(zs.data(), st->d_z.p, (size_t)N * 4, hipMemcpyDeviceToHost, st->st));
        STK_TRY(c, hipStreamSynchronize(st->st));
        classes = classify_records(recs.data(), n_calc);
        for (uint32_t q = 0; q < n_calc; ++q)
            if (classes.kept_index[q] >= 0) {
                ffs_reflection o;
                std::memcpy(&o, &recs[q], sizeof(o));
                st->out.push_back(o);
            }
        st->sig_z.resize(N);
        st->sig_refl.resize(N);
        for (uint32_t i = 0; i < N; ++i) {
            st->sig_z[i] = (int32_t)zs[i];
            st->sig_refl[i] = signal_reflection(classes, comp[i]);
        }
    }
    if (reflections) *reflections = st->out.data();
    if (n_refl) *n_refl = (uint32_t)st->out.size();
    if (n_calculated) *n_calculated = n_calc;
    if (n_f_size) *n_f_size = classes.n_too_small;
    if (n_f_sep) *n_f_sep = classes.n_too_spread;
    return FFS_OK;
}

extern "C" int ffs_stack3d_finish(ffs_stack3d* st, const ffs_reflection** reflections, uint32_t* n_refl,
                                  uint32_t* n_calculated, uint32_t* n_f_size, uint32_t* n_f_sep) {
    if (!st) return FFS_ERR_INVALID;
    return guarded(st->ctx, [&] { return stack3d_finish_impl(st, reflections, n_refl, n_calculated, n_f_size, n_f_sep); });
}
extern "C" int ffs_stack3d_last_finish_ms(const ffs_stack3d* st, float* ms) {
    if (!st || !ms) return FFS_ERR_INVALID;
    *ms = st->last_finish_ms;
    return FFS_OK;
}
