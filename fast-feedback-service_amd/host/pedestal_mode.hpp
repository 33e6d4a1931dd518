// pedestal_mode.hpp -- spotfinder --jungfrau-pedestal PREFIX: the frame source is a dark run of raw Jungfrau words; every frame is folded into
// per-pixel, per-stage accumulators (on the GPU: ffs_stream_jungfrau_pedestal_fold; with --cpu-decode on the worker threads: the host loop of
// csrc/jungfrau_pedestal_model.hpp, the same text), no spots are found, and the statistics, the planes and -- given an old calibration -- the
// re-pedestalled calibration are written as raw little-endian files.  DESIGN.md section 5e.
#pragma once
#include <vector>

#include "cli_args.hpp"
#include "reader.hpp"

namespace ffshost {

// old_calibration: the six planes of --jungfrau-calibration, or empty.  -> the process's exit code
int run_jungfrau_pedestal(const Args& args, Reader& reader, const std::vector<float>& old_calibration);

}  // namespace ffshost
