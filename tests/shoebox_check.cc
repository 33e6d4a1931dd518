// shoebox_check.cc -- csrc/shoebox_model.hpp as a plain C++ program (tests/test_shoebox_oracle.py builds it with -ffp-contract=off, plain and
// under the address and undefined-behaviour sanitizers).  shoebox_check <in> <out>
//   in:  int32 W, H, pixel bytes, n_frames, n_boxes, algorithm, has_mask, background model; int64 max_valid, first_image; float64 delta_b,
//        delta_m; the geometry (20 float64); the table (n_boxes ffs_shoebox); the mask (W*H bytes, when has_mask); the frames.
//   out: per box the accumulators (48 bytes), the histogram (256 uint32) and the record (80 bytes); then, per box and per image of the fold
//        inside its z-range, the foreground map ((x_max - x_min) * (y_max - y_min) bytes).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "launch_geometry.hpp"
#include "shoebox_model.hpp"

using namespace ffsamd;

template <typename T>
static T take(const std::vector<uint8_t>& b, size_t& at) {
    T v;
    if (at + sizeof v > b.size()) {
        std::fprintf(stderr, "shoebox_check: the input is short\n");
        std::exit(2);
    }
    std::memcpy(&v, b.data() + at, sizeof v);
    at += sizeof v;
    return v;
}

template <typename PixelT>
static void run(const ShoeboxGeometry& g, const std::vector<ShoeboxEntry>& table, int algorithm, double delta_b, double delta_m, const uint8_t* frames, int n_frames,
                int W, int H, const uint8_t* mask, uint32_t limit, int64_t first_image, int background, std::ofstream& out) {
    std::vector<uint8_t> maps;
    for (const ShoeboxEntry& b : table) {
        ShoeboxAcc acc{};
        std::vector<uint32_t> hist((size_t)kSpotBgBins, 0u);
        const size_t area = (size_t)(b.x_max - b.x_min) * (size_t)(b.y_max - b.y_min);
        for (int f = 0; f < n_frames; ++f) {
            const int64_t n = first_image + f;
            if (n < b.z_min || n >= b.z_max) continue;
            maps.resize(maps.size() + area);
            shoebox_fold_image(g, b, algorithm, delta_b, delta_m, reinterpret_cast<const PixelT*>(frames) + (size_t)f * W * H, (size_t)W, W, H, mask, limit, n, acc, hist.data(),
                               maps.data() + maps.size() - area);
        }
        const ShoeboxSum s = shoebox_sum(acc, hist.data(), background);
        out.write(reinterpret_cast<const char*>(&acc), sizeof acc);
        out.write(reinterpret_cast<const char*>(hist.data()), (std::streamsize)(hist.size() * sizeof(uint32_t)));
        out.write(reinterpret_cast<const char*>(&s), sizeof s);
    }
    out.write(reinterpret_cast<const char*>(maps.data()), (std::streamsize)maps.size());
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: shoebox_check <in> <out>\n");
        return 2;
    }
    static_assert(sizeof(ShoeboxGeometry) == 160 && sizeof(ShoeboxEntry) == 56 && sizeof(ShoeboxAcc) == 48 && sizeof(ShoeboxSum) == 80, "the layouts of the header");
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t at = 0;
    const int W = take<int32_t>(buf, at), H = take<int32_t>(buf, at), bytes = take<int32_t>(buf, at), n_frames = take<int32_t>(buf, at), n_boxes = take<int32_t>(buf, at);
    const int algorithm = take<int32_t>(buf, at), has_mask = take<int32_t>(buf, at), background = take<int32_t>(buf, at);
    const int64_t max_valid = take<int64_t>(buf, at), first_image = take<int64_t>(buf, at);
    const double delta_b = take<double>(buf, at), delta_m = take<double>(buf, at);
    const ShoeboxGeometry g = take<ShoeboxGeometry>(buf, at);
    if (W <= 0 || H <= 0 || (bytes != 2 && bytes != 4) || n_frames < 0 || n_boxes < 0) return 2;
    std::vector<ShoeboxEntry> table;
    for (int i = 0; i < n_boxes; ++i) table.push_back(take<ShoeboxEntry>(buf, at));
    const uint8_t* mask = nullptr;
    if (has_mask) {
        mask = buf.data() + at;
        at += (size_t)W * H;
    }
    if (at + (size_t)n_frames * W * H * bytes != buf.size()) {
        std::fprintf(stderr, "shoebox_check: the input's length does not fit its header\n");
        return 2;
    }
    // (the frames are copied out so that they are aligned for their pixel type)
    std::vector<uint32_t> frames(((size_t)n_frames * W * H * bytes + 3) / 4 + 1);
    std::memcpy(frames.data(), buf.data() + at, (size_t)n_frames * W * H * bytes);
    std::ofstream out(argv[2], std::ios::binary);
    const uint32_t limit = counting_limit(max_valid);
    if (bytes == 2)
        run<uint16_t>(g, table, algorithm, delta_b, delta_m, reinterpret_cast<const uint8_t*>(frames.data()), n_frames, W, H, mask, limit, first_image, background, out);
    else run<uint32_t>(g, table, algorithm, delta_b, delta_m, reinterpret_cast<const uint8_t*>(frames.data()), n_frames, W, H, mask, limit, first_image, background, out);
    return out ? 0 : 1;
}
