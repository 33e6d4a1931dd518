// ffs_index.hip -- the indexer's basis-vector search: the host-only entries ffs_index_rlp / defaults / twiddles / map / basis_vectors and the
// device entries ffs_ctx_index_grid / index_load_grid / index_peaks (include/ffs_hip.h has the definition, DESIGN.md section 3.8e the design,
// index_model.hpp the rule, index_plan.hpp the host's decisions and the buffers' sizes, kernels_index.hpp the kernels).  A device call is
// synchronous and owns what it uses: a non-blocking HIP stream, two events and the device buffers that the context keeps between calls (the
// grids per n_points, the lists grown when a call needs more, all freed with the context), under the context's index_mu, so two calls never
// overlap.  Nothing of a batch is read or written: no plan, no stream of the context's ffs_streams, no setting.
#include "ffs_internal.hpp"
#include "kernels_index.hpp"
#include "index_plan.hpp"

static_assert(sizeof(ffs_index_peak) == sizeof(IndexPeak) && offsetof(ffs_index_peak, sum) == offsetof(IndexPeak, sum) && offsetof(ffs_index_peak, frac) == offsetof(IndexPeak, frac),
              "the model's record is ffs_index_peak");
static_assert(sizeof(ffs_index_grid_stats) == sizeof(IndexGridStats) && offsetof(ffs_index_grid_stats, n_selected) == offsetof(IndexGridStats, n_selected),
              "the model's statistics are ffs_index_grid_stats");
static_assert(sizeof(ffs_index_vector) == sizeof(IndexVector) && offsetof(ffs_index_vector, volume) == offsetof(IndexVector, volume), "the model's vector is ffs_index_vector");
static_assert(sizeof(ffs_scan_geometry) == sizeof(ShoeboxGeometry), "the model's geometry is ffs_scan_geometry");

struct IndexState {
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipEvent_t lap[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // between the stages of a call: ffs_ctx_index_launch_ms
    float launch_ms[FFS_INDEX_LAUNCH_SPANS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // of the last grid call [0 .. 4] and the last peaks call [5 .. 8]
    uint32_t n_points = 0;      // what d_power, d_sums and d_tw are sized for
    uint32_t grid_points = 0;   // what d_grid is sized for
    bool resident = false;      // d_power and the sum tree in d_sums hold a grid
    IndexComplex* d_grid = nullptr;
    double *d_power = nullptr, *d_sums = nullptr, *d_tw = nullptr;   // d_sums: the tree of v | the tree of (v - mean)^2, index_sums_entries each
    uint32_t* d_cells = nullptr;
    double* d_weights = nullptr;
    uint32_t *d_counts = nullptr, *d_offsets = nullptr, *d_sel = nullptr, *d_parent = nullptr, *d_nvox = nullptr;
    unsigned long long* d_sums3 = nullptr;
    IndexPeak* d_out = nullptr;
    size_t cells_room = 0, weights_room = 0, counts_room = 0, offsets_room = 0, sel_room = 0, parent_room = 0, nvox_room = 0, sums3_room = 0, out_room = 0;   // in entries
};

void index_free_ctx(ffs_ctx* c) {
    IndexState* p = c->index;
    if (!p) return;
    if (p->st) {
        (void)hipStreamSynchronize(p->st);   // (every call has waited for its launches already)
        (void)hipStreamDestroy(p->st);
    }
    for (hipEvent_t& e : p->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t& e : p->lap)
        if (e) (void)hipEventDestroy(e);
    void* all[] = {p->d_grid, p->d_power, p->d_sums, p->d_tw, p->d_cells, p->d_weights, p->d_counts, p->d_offsets, p->d_sel, p->d_parent, p->d_nvox, p->d_sums3, p->d_out};
    for (void* d : all)
        if (d) (void)hipFree(d);
    delete p;
    c->index = nullptr;
}

// ---- host only, no context -------------------------------------------------------------------------------------------------------------------
extern "C" int ffs_index_rlp(const ffs_scan_geometry* geometry, const double* xyz_px, uint32_t n, double* rlp, double* s1, double* xyz_mm) {
    return guarded(nullptr, [&] {
        const ShoeboxGeometry* g = reinterpret_cast<const ShoeboxGeometry*>(geometry);
        const std::string why = index_rlp_refusal(g, xyz_px, n, rlp, s1, xyz_mm);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_rlp: " + why);
        for (uint32_t i = 0; i < n; ++i) index_rlp(*g, xyz_px + 3 * (size_t)i, rlp + 3 * (size_t)i, s1 + 3 * (size_t)i, xyz_mm + 3 * (size_t)i);
        return FFS_OK;
    });
}

extern "C" int ffs_index_defaults(const double* rlp, uint32_t n, double max_cell, uint32_t n_points, double* dmin, double* b_iso) {
    return guarded(nullptr, [&] {
        const std::string why = index_defaults_refusal(rlp, n, max_cell, n_points, dmin, b_iso);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_defaults: " + why);
        index_defaults(rlp, n, max_cell, n_points, *dmin, *b_iso);
        return FFS_OK;
    });
}

extern "C" int ffs_index_twiddles(uint32_t n_points, double* out) {
    return guarded(nullptr, [&] {
        const std::string why = out ? index_points_refusal(n_points) : "out is NULL";
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_twiddles: " + why);
        index_twiddles(n_points, out);
        return FFS_OK;
    });
}

extern "C" int ffs_index_map(const double* rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points, uint32_t* cell, double* weight) {
    return guarded(nullptr, [&] {
        const std::string why = (!cell || !weight) && n > 0u ? "cell or weight is NULL" : index_map_refusal(rlp, n, dmin, b_iso, n_points);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_map: " + why);
        for (uint32_t i = 0; i < n; ++i) cell[i] = index_map_one(rlp + 3 * (size_t)i, dmin, b_iso, n_points, weight[i]);
        return FFS_OK;
    });
}

extern "C" int ffs_index_basis_vectors(const ffs_index_peak* peaks, uint32_t n, uint32_t n_points, double dmin, double peak_volume_cutoff, double min_cell, double max_cell,
                                       ffs_index_vector* out, uint32_t cap, uint32_t* n_out) {
    return guarded(nullptr, [&] {
        const IndexPeak* p = reinterpret_cast<const IndexPeak*>(peaks);
        const std::string why = index_basis_refusal(p, n, n_points, dmin, peak_volume_cutoff, min_cell, max_cell, !out, cap, !n_out);
        if (!why.empty()) return refuse(g_create_error, FFS_ERR_INVALID, "ffs_index_basis_vectors: " + why);
        const std::vector<IndexVector> v = index_basis_vectors(p, n, n_points, dmin, peak_volume_cutoff, min_cell, max_cell);
        *n_out = (uint32_t)v.size();
        const size_t take = std::min<size_t>(v.size(), cap);
        if (take) std::memcpy(out, v.data(), take * sizeof(IndexVector));
        if (v.size() > cap) return refuse(g_create_error, FFS_ERR_OVERFLOW, "ffs_index_basis_vectors: " + std::to_string(v.size()) + " vectors do not fit cap " + std::to_string(cap));
        return FFS_OK;
    });
}

// ---- device ------------------------------------------------------------------------------------------------------------------------------------
// room for `want` entries behind *p (kept when it is there already)
template <typename T>
static int index_room(ffs_ctx* c, const char* who, T** p, size_t& room, size_t want, const char* what) {
    if (want <= room) return FFS_OK;
    if (*p) HIP_TRY(c, hipFree(*p));
    *p = nullptr, room = 0;
    if (dmalloc(p, want * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return refuse(c->err, FFS_ERR_NOMEM, std::string(who) + what + " (" + std::to_string((want * sizeof(T)) >> 20) + " MB) do not fit");
    }
    room = want;
    return FFS_OK;
}

// the stream, the events and the buffers of a grid of n points a side (the complex grid only for ffs_ctx_index_grid)
static int index_prepare(ffs_ctx* c, const char* who, uint32_t n, bool complex_grid) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->index) c->index = new IndexState;
    IndexState* p = c->index;
    if (!p->st) HIP_TRY(c, hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
    for (hipEvent_t& e : p->ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    for (hipEvent_t& e : p->lap)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    if (p->n_points != n) {
        p->resident = false;
        for (double** d : {&p->d_power, &p->d_sums, &p->d_tw})
            if (*d) {
                HIP_TRY(c, hipFree(*d));
                *d = nullptr;
            }
        p->n_points = 0;
        size_t room = 0;
        FFS_TRY(index_room(c, who, &p->d_power, room, index_voxels(n), "the power grid"));
        room = 0;
        FFS_TRY(index_room(c, who, &p->d_sums, room, 2 * index_sums_entries(n), "the sums"));
        room = 0;
        FFS_TRY(index_room(c, who, &p->d_tw, room, (size_t)n, "the twiddles"));
        std::vector<double> tw(n);
        index_twiddles(n, tw.data());
        // (in the call's own stream and waited for here, while `tw` lives: no other stream of the process is made to wait)
        HIP_TRY(c, hipMemcpyAsync(p->d_tw, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
        HIP_TRY(c, hipStreamSynchronize(p->st));
        p->n_points = n;
    }
    if (complex_grid && p->grid_points != n) {
        if (p->d_grid) HIP_TRY(c, hipFree(p->d_grid));
        p->d_grid = nullptr, p->grid_points = 0;
        size_t room = 0;
        FFS_TRY(index_room(c, who, &p->d_grid, room, index_voxels(n), "the complex grid"));
        p->grid_points = n;
    }
    return FFS_OK;
}

#define INDEX_FOR_N(n, CALL)                 \
    switch (n) {                             \
        case 16u: { CALL(16u); break; }      \
        case 32u: { CALL(32u); break; }      \
        case 64u: { CALL(64u); break; }      \
        case 128u: { CALL(128u); break; }    \
        default: { CALL(256u); break; }      \
    }

static constexpr uint32_t kWavesPerBlock = (uint32_t)kIndexThreads / 64u;

// lines (already in sums[0 .. N^2)) to planes to the total
static void index_launch_trees(IndexState* p, double* sums, uint32_t n) {
#define TREES(N)                                                                                                                                     \
    hipLaunchKernelGGL(k_index_tree<N>, dim3((N + kWavesPerBlock - 1u) / kWavesPerBlock), dim3(kIndexThreads), 0, p->st, sums, sums + (size_t)N * N, N); \
    hipLaunchKernelGGL(k_index_tree<N>, dim3(1), dim3(kIndexThreads), 0, p->st, sums + (size_t)N * N, sums + (size_t)N * N + N, 1u)
    INDEX_FOR_N(n, TREES)
#undef TREES
}

static int index_grid_impl(ffs_ctx* c, const double* rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points, uint8_t* used, double* power_out, float* kernel_ms) {
    static const char* who = "ffs_ctx_index_grid: ";
    if (kernel_ms) *kernel_ms = 0.0f;
    const std::string why = index_map_refusal(rlp, n, dmin, b_iso, n_points);
    if (!why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + why);
    std::vector<uint32_t> cell(n), cells;
    std::vector<double> weight(n), weights;
    for (uint32_t i = 0; i < n; ++i) cell[i] = index_map_one(rlp + 3 * (size_t)i, dmin, b_iso, n_points, weight[i]);
    index_map_dedup(cell.data(), weight.data(), n, cells, weights);

    std::lock_guard<std::mutex> lock(c->index_mu);
    FFS_TRY(index_prepare(c, who, n_points, true));
    IndexState* p = c->index;
    p->resident = false;
    const uint32_t n_cells = (uint32_t)cells.size();
    FFS_TRY(index_room(c, who, &p->d_cells, p->cells_room, cells.size(), "the cells"));
    FFS_TRY(index_room(c, who, &p->d_weights, p->weights_room, weights.size(), "the weights"));
    (void)hipGetLastError();
    if (n_cells) {
        HIP_TRY(c, hipMemcpyAsync(p->d_cells, cells.data(), cells.size() * sizeof(uint32_t), hipMemcpyHostToDevice, p->st));
        HIP_TRY(c, hipMemcpyAsync(p->d_weights, weights.data(), weights.size() * sizeof(double), hipMemcpyHostToDevice, p->st));
    }
    HIP_TRY(c, hipEventRecord(p->lap[0], p->st));
    HIP_TRY(c, hipMemsetAsync(p->d_grid, 0, index_complex_bytes(n_points), p->st));
    if (n_cells) hipLaunchKernelGGL(k_index_scatter, dim3((n_cells + kIndexThreads - 1) / kIndexThreads), dim3(kIndexThreads), 0, p->st, p->d_grid, p->d_cells, p->d_weights, n_cells);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p->lap[1], p->st));
    IndexFftArgs a{p->d_grid, p->d_tw, p->d_power, p->d_sums};
    const uint32_t blocks = index_fft_blocks(n_points);
#define PASSES(N)                                                                                        \
    hipLaunchKernelGGL((k_index_fft<N, 0>), dim3(blocks), dim3(kIndexThreads), 0, p->st, a);             \
    (void)hipEventRecord(p->lap[2], p->st);                                                              \
    hipLaunchKernelGGL((k_index_fft<N, 1>), dim3(blocks), dim3(kIndexThreads), 0, p->st, a);             \
    (void)hipEventRecord(p->lap[3], p->st);                                                              \
    hipLaunchKernelGGL((k_index_fft<N, 2>), dim3(blocks), dim3(kIndexThreads), 0, p->st, a);             \
    (void)hipEventRecord(p->lap[4], p->st)
    INDEX_FOR_N(n_points, PASSES)
#undef PASSES
    HIP_TRY(c, hipGetLastError());
    index_launch_trees(p, p->d_sums, n_points);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p->lap[5], p->st));
    if (power_out) HIP_TRY(c, hipMemcpyAsync(power_out, p->d_power, index_power_bytes(n_points), hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipStreamSynchronize(p->st));
    // fill + scatter | FFT axis 0 | axis 1 | axis 2 with the power grid and the line sums | the sums' trees
    for (int k = 0; k < 5; ++k) HIP_TRY(c, hipEventElapsedTime(&p->launch_ms[k], p->lap[k], p->lap[k + 1]));
    if (kernel_ms) HIP_TRY(c, hipEventElapsedTime(kernel_ms, p->lap[0], p->lap[5]));
    p->resident = true;
    if (used)
        for (uint32_t i = 0; i < n; ++i) used[i] = cell[i] != kIndexNotUsed ? 1 : 0;
    return FFS_OK;
}

static int index_load_impl(ffs_ctx* c, const double* power, uint32_t n_points) {
    static const char* who = "ffs_ctx_index_load_grid: ";
    const std::string why = index_load_refusal(power, n_points);
    if (!why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + why);
    std::lock_guard<std::mutex> lock(c->index_mu);
    FFS_TRY(index_prepare(c, who, n_points, false));
    IndexState* p = c->index;
    p->resident = false;
    (void)hipGetLastError();
    HIP_TRY(c, hipMemcpyAsync(p->d_power, power, index_power_bytes(n_points), hipMemcpyHostToDevice, p->st));
    const uint32_t line_blocks = n_points * n_points / kWavesPerBlock;
#define LINES(N) hipLaunchKernelGGL((k_index_lines<N, false>), dim3(line_blocks), dim3(kIndexThreads), 0, p->st, p->d_power, p->d_sums, p->d_sums)
    INDEX_FOR_N(n_points, LINES)
#undef LINES
    HIP_TRY(c, hipGetLastError());
    index_launch_trees(p, p->d_sums, n_points);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(p->st));
    p->resident = true;
    return FFS_OK;
}

static int index_peaks_impl(ffs_ctx* c, double rmsd_cutoff, ffs_index_peak* out, uint32_t cap, uint32_t* n, ffs_index_grid_stats* stats, float* kernel_ms) {
    static const char* who = "ffs_ctx_index_peaks: ";
    if (kernel_ms) *kernel_ms = 0.0f;
    std::lock_guard<std::mutex> lock(c->index_mu);
    IndexState* p = c->index;
    const std::string why = index_peaks_refusal(rmsd_cutoff, !out, cap, !n, p && p->resident ? p->n_points : 0u);
    if (!why.empty()) return refuse(c->err, FFS_ERR_INVALID, who + why);
    HIP_TRY(c, hipSetDevice(c->device));
    (void)hipGetLastError();
    const uint32_t N = p->n_points;
    const size_t entries = index_sums_entries(N);
    double* ssq = p->d_sums + entries;
    float ms_sum = 0.0f, ms = 0.0f;
    // the second statistic: the mean is taken on the device from the total it holds
    HIP_TRY(c, hipEventRecord(p->ev[0], p->st));
    const uint32_t line_blocks = N * N / kWavesPerBlock;
#define LINES(NN) hipLaunchKernelGGL((k_index_lines<NN, true>), dim3(line_blocks), dim3(kIndexThreads), 0, p->st, p->d_power, p->d_sums + entries - 1, ssq)
    INDEX_FOR_N(N, LINES)
#undef LINES
    HIP_TRY(c, hipGetLastError());
    index_launch_trees(p, ssq, N);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p->ev[1], p->st));
    double totals[2] = {0.0, 0.0};
    HIP_TRY(c, hipMemcpyAsync(&totals[0], p->d_sums + entries - 1, sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipMemcpyAsync(&totals[1], ssq + entries - 1, sizeof(double), hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipStreamSynchronize(p->st));
    HIP_TRY(c, hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    ms_sum += ms;
    for (int k = 5; k < FFS_INDEX_LAUNCH_SPANS; ++k) p->launch_ms[k] = 0.0f;
    p->launch_ms[5] = ms;   // the second statistic
    IndexGridStats st{};
    index_stats_finish(st, totals[0], totals[1], N, rmsd_cutoff);

    // the selection: count, scan, (the list sized from the count,) write
    IndexListArgs a{};
    a.power = p->d_power, a.cutoff = st.cutoff, a.n_points = N, a.n_blocks = index_select_blocks(N);
    // (counts and offsets for either count pass: the selection's N^3 / 4096 workgroups, the roots' at most N^3 / 256)
    FFS_TRY(index_room(c, who, &p->d_counts, p->counts_room, (size_t)index_list_blocks((uint32_t)index_voxels(N)), "the workgroups' counts"));
    FFS_TRY(index_room(c, who, &p->d_offsets, p->offsets_room, (size_t)index_list_blocks((uint32_t)index_voxels(N)) + 1, "the workgroups' offsets"));
    a.counts = p->d_counts, a.offsets = p->d_offsets;
    HIP_TRY(c, hipEventRecord(p->ev[0], p->st));
    hipLaunchKernelGGL(k_index_select_count, dim3(a.n_blocks), dim3(kIndexThreads), 0, p->st, a);
    hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kIndexScanThreads), 0, p->st, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(p->ev[1], p->st));
    uint32_t n_sel = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_sel, p->d_offsets + a.n_blocks, sizeof n_sel, hipMemcpyDeviceToHost, p->st));
    HIP_TRY(c, hipStreamSynchronize(p->st));
    HIP_TRY(c, hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    ms_sum += ms;
    p->launch_ms[6] = ms;   // the selection's count and scan (its write pass is added below)
    st.n_selected = n_sel;
    uint32_t n_roots = 0;
    if (n_sel) {
        FFS_TRY(index_room(c, who, &p->d_sel, p->sel_room, (size_t)n_sel, "the selected voxels"));
        FFS_TRY(index_room(c, who, &p->d_parent, p->parent_room, (size_t)n_sel, "the selected voxels' parents"));
        FFS_TRY(index_room(c, who, &p->d_nvox, p->nvox_room, (size_t)n_sel, "the components' counts"));
        FFS_TRY(index_room(c, who, &p->d_sums3, p->sums3_room, 3 * (size_t)n_sel, "the components' sums"));
        a.n = n_sel, a.sel = p->d_sel, a.parent = p->d_parent, a.n_voxels = p->d_nvox, a.sums = p->d_sums3;
        const uint32_t list_blocks = index_list_blocks(n_sel);
        IndexListArgs r = a;   // the roots' count pass has its own number of workgroups
        r.n_blocks = list_blocks;
        HIP_TRY(c, hipEventRecord(p->ev[0], p->st));
        hipLaunchKernelGGL(k_index_select_write, dim3(a.n_blocks), dim3(kIndexThreads), 0, p->st, a);
        (void)hipEventRecord(p->lap[0], p->st);
        hipLaunchKernelGGL(k_index_union, dim3(list_blocks), dim3(kIndexThreads), 0, p->st, a);
        hipLaunchKernelGGL(k_index_flatten, dim3(list_blocks), dim3(kIndexThreads), 0, p->st, a);
        (void)hipEventRecord(p->lap[1], p->st);
        hipLaunchKernelGGL(k_index_reduce, dim3(list_blocks), dim3(kIndexThreads), 0, p->st, a);
        hipLaunchKernelGGL(k_index_root_count, dim3(list_blocks), dim3(kIndexThreads), 0, p->st, r);
        hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kIndexScanThreads), 0, p->st, r);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(p->ev[1], p->st));
        HIP_TRY(c, hipMemcpyAsync(&n_roots, p->d_offsets + list_blocks, sizeof n_roots, hipMemcpyDeviceToHost, p->st));
        HIP_TRY(c, hipStreamSynchronize(p->st));
        HIP_TRY(c, hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
        ms_sum += ms;
        float part = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&part, p->ev[0], p->lap[0]));
        p->launch_ms[6] += part;   // the selection's write pass
        HIP_TRY(c, hipEventElapsedTime(&p->launch_ms[7], p->lap[0], p->lap[1]));   // union and flatten
        HIP_TRY(c, hipEventElapsedTime(&p->launch_ms[8], p->lap[1], p->ev[1]));    // per-root sums, the roots' count and scan (their write is added below)
        const uint32_t take = std::min(n_roots, cap);
        if (take) {
            FFS_TRY(index_room(c, who, &p->d_out, p->out_room, (size_t)take, "the records"));
            r.out = p->d_out, r.cap = take;
            HIP_TRY(c, hipEventRecord(p->ev[0], p->st));
            hipLaunchKernelGGL(k_index_root_write, dim3(list_blocks), dim3(kIndexThreads), 0, p->st, r);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipEventRecord(p->ev[1], p->st));
            HIP_TRY(c, hipMemcpyAsync(out, p->d_out, (size_t)take * sizeof(IndexPeak), hipMemcpyDeviceToHost, p->st));
            HIP_TRY(c, hipStreamSynchronize(p->st));
            HIP_TRY(c, hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
            ms_sum += ms;
            p->launch_ms[8] += ms;
        }
    }
    st.n_peaks = n_roots;
    *n = n_roots;
    if (stats) std::memcpy(stats, &st, sizeof st);
    if (kernel_ms) *kernel_ms = ms_sum;
    if (n_roots > cap) return refuse(c->err, FFS_ERR_OVERFLOW, who + std::to_string(n_roots) + " records do not fit cap " + std::to_string(cap));
    return FFS_OK;
}

extern "C" int ffs_ctx_index_grid(ffs_ctx* c, const double* rlp, uint32_t n, double dmin, double b_iso, uint32_t n_points, uint8_t* used, double* power_out, float* kernel_ms) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return index_grid_impl(c, rlp, n, dmin, b_iso, n_points, used, power_out, kernel_ms); });
}

extern "C" int ffs_ctx_index_load_grid(ffs_ctx* c, const double* power, uint32_t n_points) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return index_load_impl(c, power, n_points); });
}

extern "C" int ffs_ctx_index_peaks(ffs_ctx* c, double rmsd_cutoff, ffs_index_peak* out, uint32_t cap, uint32_t* n, ffs_index_grid_stats* stats, float* kernel_ms) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] { return index_peaks_impl(c, rmsd_cutoff, out, cap, n, stats, kernel_ms); });
}

extern "C" int ffs_ctx_index_launch_ms(ffs_ctx* c, float* out) {
    if (!c) return FFS_ERR_INVALID;
    return guarded(c, [&] {
        if (!out) return refuse(c->err, FFS_ERR_INVALID, "ffs_ctx_index_launch_ms: out is NULL");
        std::lock_guard<std::mutex> lock(c->index_mu);
        for (int k = 0; k < FFS_INDEX_LAUNCH_SPANS; ++k) out[k] = c->index ? c->index->launch_ms[k] : 0.0f;
        return FFS_OK;
    });
}
