// predict_check.cc -- csrc/predict_model.hpp and csrc/predict_plan.hpp as a plain C++ program (tests/test_predict_oracle.py builds it with
// -ffp-contract=off, plain and under the address and undefined-behaviour sanitizers).  predict_check <in> <out>
//   in:  int32 W, H, n_images, centring, has_settings, 0; float64 dmin, delta_b, delta_m; the geometry (20 float64); the a_matrix
//        (9 float64); when has_settings, (n_images + 1) * 9 float64 scan-point settings to predict with.
//   out: int32 h_max[3], uint32 n_candidates, uint32 n_records, uint32 0; the scan-point settings this program computes itself
//        ((n_images + 1) * 9 float64); the records (96 bytes each), predicted with the given settings when there are some, else with its own.
//   A refused call writes nothing and prints the refusal; exit status 3.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "predict_plan.hpp"

using namespace ffsamd;

template <typename T>
static T take(const std::vector<uint8_t>& b, size_t& at) {
    T v;
    if (at + sizeof v > b.size()) {
        std::fprintf(stderr, "predict_check: the input is short\n");
        std::exit(2);
    }
    std::memcpy(&v, b.data() + at, sizeof v);
    at += sizeof v;
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: predict_check <in> <out>\n");
        return 2;
    }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t at = 0;
    const int W = take<int32_t>(buf, at), H = take<int32_t>(buf, at);
    const uint32_t n_images = take<uint32_t>(buf, at);
    PredictCrystal x{};
    x.centring = take<int32_t>(buf, at);
    const int has_settings = take<int32_t>(buf, at);
    (void)take<int32_t>(buf, at);
    const double dmin = take<double>(buf, at), delta_b = take<double>(buf, at), delta_m = take<double>(buf, at);
    const ShoeboxGeometry g = take<ShoeboxGeometry>(buf, at);
    for (double& v : x.a_matrix) v = take<double>(buf, at);
    PredictSetup u;
    const std::string why = predict_refusal(g, x, n_images, dmin, delta_b, delta_m, W, H, u);
    if (!why.empty()) {
        std::printf("%s\n", why.c_str());
        return 3;
    }
    std::vector<double> own(((size_t)n_images + 1) * 9), given;
    predict_scan_settings(g, x.a_matrix, n_images, own.data());
    if (has_settings)
        for (size_t i = 0; i < own.size(); ++i) given.push_back(take<double>(buf, at));
    if (at != buf.size()) {
        std::fprintf(stderr, "predict_check: the input's length does not fit its header\n");
        return 2;
    }
    std::vector<PredictRecord> records;
    predict_all(u, has_settings ? given.data() : own.data(), records);
    std::ofstream out(argv[2], std::ios::binary);
    const uint32_t head[3] = {u.n_candidates, (uint32_t)records.size(), 0u};
    out.write(reinterpret_cast<const char*>(u.h_max), sizeof u.h_max);
    out.write(reinterpret_cast<const char*>(head), sizeof head);
    out.write(reinterpret_cast<const char*>(own.data()), (std::streamsize)(own.size() * sizeof(double)));
    out.write(reinterpret_cast<const char*>(records.data()), (std::streamsize)(records.size() * sizeof(PredictRecord)));
    return out ? 0 : 1;
}
