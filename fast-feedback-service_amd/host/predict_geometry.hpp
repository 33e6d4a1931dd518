// predict_geometry.hpp -- what spotfinder --predict hands to ffs_ctx_predict besides the flat geometry of shoebox_geometry.hpp: the crystal
// file, the centring letter, the summary line and the table of boxes taken from the predictions.  `ffs_hosttool predict` and
// `ffs_hosttool shoebox predictions=` call the same text, so a test can hold the driver to it.
//
// The crystal file: nine raw little-endian float64, the A matrix row-major in 1/Angstrom (r = A h in the laboratory frame at rotation
// angle 0, fixed and setting rotations applied).
#pragma once
#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ffs_hip.h"

namespace ffshost {

inline int centring_from_letter(const std::string& s) {
    static const char* letters = "PIFABCR";
    if (s.size() == 1)
        for (int i = 0; letters[i]; ++i)
            if (letters[i] == s[0]) return i;
    throw std::runtime_error("the centring must be one of P I F A B C R, got " + s);
}

inline ffs_crystal read_crystal_file(const std::string& path, int centring) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the crystal file " + path);
    ffs_crystal x{};
    f.read(reinterpret_cast<char*>(x.a_matrix), sizeof x.a_matrix);
    if (f.gcount() != (std::streamsize)sizeof x.a_matrix || f.peek() != std::ifstream::traits_type::eof())
        throw std::runtime_error("the crystal file " + path + " is not nine float64 (72 bytes)");
    x.centring = centring;
    return x;
}

inline std::vector<ffs_prediction> read_prediction_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the prediction file " + path);
    f.seekg(0, std::ios::end);
    const std::streamoff bytes = f.tellg();
    f.seekg(0);
    if (bytes < 0 || bytes % (std::streamoff)sizeof(ffs_prediction) != 0)
        throw std::runtime_error("the prediction file " + path + " is not a whole number of 96-byte records (" + std::to_string((long long)bytes) + " bytes)");
    std::vector<ffs_prediction> recs((size_t)bytes / sizeof(ffs_prediction));
    if (!recs.empty()) f.read(reinterpret_cast<char*>(recs.data()), bytes);
    if (!f) throw std::runtime_error("short read of the prediction file " + path);
    return recs;
}

// The boxes a shoebox job is opened with: those of the records not flagged FFS_PREDICT_BOX_REFUSED, in their order
inline std::vector<ffs_shoebox> boxes_of_predictions(const std::vector<ffs_prediction>& p) {
    std::vector<ffs_shoebox> out;
    for (const ffs_prediction& r : p)
        if (!(r.flags & FFS_PREDICT_BOX_REFUSED)) out.push_back(r.box);
    return out;
}

// The summary line of a prediction: candidates, predictions, and the records with a flag other than FFS_PREDICT_ENTERING
inline std::string predict_summary_line(uint64_t n_candidates, const std::vector<ffs_prediction>& p) {
    size_t flagged = 0;
    for (const ffs_prediction& r : p) flagged += (r.flags & ~FFS_PREDICT_ENTERING) != 0;
    return "prediction: " + std::to_string(n_candidates) + " candidates, " + std::to_string(p.size()) + " predictions, " + std::to_string(flagged) + " flagged";
}

}  // namespace ffshost
