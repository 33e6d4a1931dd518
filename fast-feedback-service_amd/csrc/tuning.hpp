// tuning.hpp -- the tuning values of a context (ffs_ctx_set_tuning).  Plain integers, no HIP header: ffs_internal.hpp includes it, and so
// does launch_geometry.hpp, whose arithmetic reads four of them.
#pragma once

namespace ffsamd {

// ---- tuning ---------------------------------------------------------------------------------------------------
// Every setting here selects between paths that give the SAME results (A/B partners, fall-backs, capacities that
// tests shrink); they are set per context through ffs_ctx_set_tuning(), never through the environment.  The timing
// experiments that break results exist only in -DFFS_EXPERIMENTS builds (`exp`, read from FFS_EXP_* there).
struct Tuning {
    int threshold_path = 0;     // 0: bright windows -> list -> k_bright_fix; 1: bright windows -> plane -> k_exact (also the
                                //    fall-back when the list overflows); 2: no streaming kernel at all -- EVERY valid pixel is a candidate
                                //    and k_exact gathers its window (the independent partner of `spotfinder --validate`; ~10 ms per frame)
    int ext_first_pass = 2;     // extended algorithm, 16-bit pixels: 2 = streaming kernel, 0 = k_ext_first
    int sparse_stage = 2;       // one launch per batch, a workgroup per frame (k_frame_chain): 3 = always, 2 = unless the stream's previous
                                //    batch held a frame beyond its LDS forest; 1 = four grid-wide kernels
    int sched = 3;              // 3 = the context's streams share one dense, two sparse and one upload HIP stream; 0 = one HIP stream per ffs_stream
    int chain_first = 2;        // while at most n batches are in flight the sparse launch does the bright fix-up and the next
                                //    streaming kernel waits for its start; 0 = never
    int bright_cap = 1 << 20;   // entries of the bright-window list actually used
    int frames_per_group = 1 << 30;   // frames side by side in one super row of the streaming kernels (cap)
    long long target_waves = 16384;   // waves a streaming launch aims for
    int stream_bands = 0;             // > 0: bands of a streaming launch (0: from target_waves, a multiple of eight of at least 72 rows)
    int dense_mask = 0;         // 1: always produce the dense byte mask
    int occupancy_bitmap = 1;   // k_frame_chain reads only the plane segments the occupancy bitmap names
    int direct_records = 1;     // records and counters are written straight into pinned host memory
    int decode_in_dense_stream = 1;   // the decode kernel runs in the dense kernels' stream (0: in the upload stream)
    int ccl_grid = 32;          // workgroups per frame of the grid-wide sparse kernels
    int ext_erode = 2;          // extended algorithm, erosion: 0 = k_ext_erode (a lane per word column, three loads per row), 1 / 2 = k_ext_erode_strips
                                //    (a wave per 62 word columns and 32 / 16 rows, one load per row, neighbours by DPP; non-zero words only
                                //    when the plane was cleared behind the previous batch)
    int ext_e_sparse = 0;       // ... 1 = the signal-region plane is cleared behind the previous batch and the strip erosion stores its non-zero words only
    int ext_fused = 0;          // extended algorithm, 16-bit pixels: 1 = erosion fused into the final pass's tiles (k_ext_erode_final: one launch, the plane
                                //    crosses memory once); 0 = k_ext_erode + k_ext_final.  Measured round 4: the fused kernel is SLOWER (threshold stage 0.65
                                //    against 0.55 ms per 32 frames, profiles/r04d_ext_fused_ab.txt): every tile starts with a chain of dependent plane loads
                                //    that its gathers then wait behind, 17 000 times per batch -- kept as an A/B partner, parity-tested
    int ext_rest_aside = 0;     // extended algorithm: 1 = erosion + final pass in the batch's sparse stream, beside the next batch's first pass; 0 = in the
                                //    dense stream (measured round 4: no gain -- a CU full of first-pass waves has neither LDS nor registers left for the
                                //    final pass's workgroups, so the kernels take turns either way: profiles/r04b_ext_streams_ab.txt)
    int band_taper = 0;         // streaming kernels: the last two bands per XCD are this many per cent as tall as the others (0 = uniform bands)
    int rows_ahead = 3;         // rows of loads a wave of the streaming kernels keeps in flight (16-bit pixels: 2, 3 or 4; 32-bit: 2 or 3).  Round 5: three.
                                //    Alone the kernel is the same with two (round 4's measurement, and why it was two); in the pipeline, beside the
                                //    band launches, three is 5 % faster (0.292-0.296 against 0.309-0.312 ms: profiles/r05zj_rows_ahead_ab.log)
    int device_lists = 2;       // the strong-pixel lists stay on the device after a batch: 1 = always, 0 = only when the host asked for them
                                //    (want_strong_list), 2 = also while a 3D stack of the process is alive (ffs_stack3d_add_batch reads them)
    int strong_log = 1;         // 16-bit standard path: the streaming kernel appends its strong groups to per-wave logs and the one-launch sparse
                                //    stage merges them (kernels_chain.hpp, LOG) instead of scattering plane bytes, counters and occupancy bits;
                                //    0 = the bit plane (also what dense frames, tall frames and the other algorithms and paths take)
    int chain_runs = 1;         // sparse_stage 2: frames beyond the LDS forest of pixels stay in the one launch when their RUNS fit
                                //    (16-bit pixels, rows up to 16383 pixels); 0 = such batches take the four grid-wide kernels; 2 = runs for every frame
    int sparse_bands = 1;       // standard path with wave logs, lists not asked for: the sparse stage in small workgroups (kernels_band.hpp: a wave per
                                //    band of a frame + a merge per frame) instead of k_frame_chain's one workgroup per frame: 1 = with one or with four
                                //    and more batches in flight (measured: ffs_submit.hip), 2 = always, 0 = never
    int dense_overlap = 0;      // wave-log path: 1 = consecutive streaming kernels on two HIP streams, handed over by a value the launch's last workgroup
                                //    writes as it starts (hipStreamWaitValue32); 0 = one dense stream, a barrier between its dispatches.  Measured round 5:
                                //    the idea works in isolation (tools/ubench/wait_value.hip: 159 -> 146 us per launch of 15 064 sleeping waves) and LOSES
                                //    8-10 % in the pipeline (0.335-0.35 against 0.307-0.313 ms per step, four or eight hardware queues:
                                //    profiles/r05t_dense_overlap_ab.log) -- the next kernel's first waves and the band launches then fight over the same
                                //    freed slots, and each streaming kernel takes 0.325 instead of 0.298 ms.  Off; kept as the A/B partner
    int stream_prio = 1;        // 1: the 16-bit streaming kernel's waves run at issue priority 3 (s_setprio), ahead of the band waves that share their SIMDs
                                //    (+1 % on the driver-style line, six alternating pairs: profiles/r05zm_stream_prio_ab.log); 0: default priority
    int assembly_threads = 7;   // helper threads that assemble a batch's result arrays beside the caller (made with the context's first large batch)
    int wait_ahead = 1;         // a thread of the context assembles each batch's result arrays as soon as the GPU has finished it (0: ffs_wait does)
    int sparse_priority = 0;    // priority of the context's sparse HIP streams: 0 = highest, 1 = lowest, 2 = the dense stream's
    int window_kernel = 0;      // 1: the general-window kernel (kernels_window.hpp) also runs the 7x7 window -- the A/B and cross-check partner
                                //    of k_stream_u16 / k_stream_u32; 0: only windows other than 3,3 take it
    int radial_stream = 0;      // the radial profile's two launches (kernels_radial.hpp): 0 = in the batch's sparse stream behind its sparse launch, 1 = in the
                                //    dense stream behind the threshold stage's kernels (the A/B partner: DESIGN.md section 3.6 has both measurements)
    int radial_map8 = 0;        // k_radial reads the bin map in one byte an entry where the map has at most 255 bins (1) or always in two (0)
    int stats_stream = 0;       // the per-pixel statistics' launch (kernels_pixstats.hpp): 0 = in a HIP stream of the context's own, beside the batch's threshold
                                //    stage, 1 = in the dense stream behind the threshold stage's kernels (the A/B partner: DESIGN.md section 3.7)
    int radthr_bands = 0;       // the radial-profile threshold's histogram launch (kernels_radthr.hpp): 0 = the launch chooses its bands per frame, > 0 = that
                                //    many, clamped to 1..H (tests put the band seams where they want them)
    int radthr_form = 0;        // ... and how a lane's counts meet the workgroup's table: 1 = one LDS add per counting pixel, 2 = a run of equal (shell, value)
                                //    pairs kept in registers, 0 = what measured faster for the pixel size: 2 for 16-bit pixels, 1 for 32-bit
#ifdef FFS_EXPERIMENTS
    struct Exp {
        int k1_debug = 0, chain_skip = 0, chain_stop = 0, dummy_us = 0, dummy_wg = 32, dummy_threads = 1024, dummy_lds = 0;
    } exp;
#endif
};

}  // namespace ffsamd
