// png_writer.hpp -- what --writeout draws: the masks and, per image, the grey frame with its spots' boxes and strong pixels
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "ffs_hip.h"

namespace ffshost {

// minimal PNG (stored deflate blocks) for --writeout, in place of lodepng
inline void write_png_rgb(const std::string& path, const uint8_t* rgb, uint32_t w, uint32_t h) {
    auto crc32 = [](const uint8_t* d, size_t n, uint32_t c) {
        static uint32_t table[256];
        static bool init = false;
        if (!init) {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t k = i;
                for (int j = 0; j < 8; ++j) k = (k & 1) ? 0xEDB88320u ^ (k >> 1) : k >> 1;
                table[i] = k;
            }
            init = true;
        }
        c = ~c;
        for (size_t i = 0; i < n; ++i) c = table[(c ^ d[i]) & 255] ^ (c >> 8);
        return ~c;
    };
    std::ofstream f(path, std::ios::binary);
    auto be32 = [](uint32_t v, uint8_t* o) { o[0] = v >> 24; o[1] = v >> 16; o[2] = v >> 8; o[3] = v; };
    auto chunk = [&f, &be32, &crc32](const char* type, const std::vector<uint8_t>& data) {
        uint8_t len[4];
        be32((uint32_t)data.size(), len);
        f.write((const char*)len, 4);
        std::vector<uint8_t> td(type, type + 4);
        td.insert(td.end(), data.begin(), data.end());
        f.write((const char*)td.data(), (std::streamsize)td.size());
        uint8_t c[4];
        be32(crc32(td.data(), td.size(), 0), c);
        f.write((const char*)c, 4);
    };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    f.write((const char*)sig, 8);
    std::vector<uint8_t> ihdr(13);
    be32(w, &ihdr[0]);
    be32(h, &ihdr[4]);
    ihdr[8] = 8; ihdr[9] = 2; ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
    chunk("IHDR", ihdr);
    std::vector<uint8_t> raw;
    raw.reserve((size_t)h * (3 * w + 1));
    for (uint32_t y = 0; y < h; ++y) {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + (size_t)y * w * 3, rgb + (size_t)(y + 1) * w * 3);
    }
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0;
    for (size_t off = 0; off < raw.size();) {
        const size_t n = std::min<size_t>(65535, raw.size() - off);
        z.push_back(off + n == raw.size() ? 1 : 0);
        z.push_back(n & 255); z.push_back(n >> 8); z.push_back(~n & 255); z.push_back((~n >> 8) & 255);
        z.insert(z.end(), raw.begin() + off, raw.begin() + off + n);
        for (size_t i = 0; i < n; ++i) { a = (a + raw[off + i]) % 65521; b = (b + a) % 65521; }
        off += n;
    }
    uint8_t ad[4];
    be32((b << 16) | a, ad);
    z.insert(z.end(), ad, ad + 4);
    chunk("IDAT", z);
    chunk("IEND", {});
}

inline void write_mask_png(const std::string& path, const uint8_t* mask, uint32_t w, uint32_t h) {
    std::vector<uint8_t> img((size_t)w * h * 3, 255);  // spotfinder.cc:627-645
    for (size_t k = 0; k < (size_t)w * h; ++k)
        if (!mask[k]) { img[3 * k + 1] = 0; img[3 * k + 2] = 0; }
    write_png_rgb(path, img.data(), w, h);
}

// image_%05u.png and pixels_%05u.txt of one frame (spotfinder.cc:937-994): the pixels in grey, frames around the spots'
// boxes in blue, strong pixels in red and listed as "x, y" lines
inline void write_overlay(const ffs_frame_result& r, const uint8_t* px, size_t bytes_per_pixel, uint32_t width, uint32_t height) {
    const uint32_t image_num = (uint32_t)r.frame_id;
    std::vector<uint8_t> img((size_t)width * height * 3);
    for (size_t k = 0; k < (size_t)width * height; ++k) {
        const float v = bytes_per_pixel == 2 ? (float)reinterpret_cast<const uint16_t*>(px)[k]
                                             : (float)reinterpret_cast<const uint32_t*>(px)[k];
        const uint8_t g = (uint8_t)std::max(0.0f, 255.99f - v * 10);
        img[3 * k] = img[3 * k + 1] = img[3 * k + 2] = g;
    }
    auto put = [&img, width, height](long x, long y) {
        if (x >= 0 && y >= 0 && x < (long)width && y < (long)height) {
            const size_t k = (size_t)y * width + x;
            img[3 * k] = 0; img[3 * k + 1] = 0; img[3 * k + 2] = 255;
        }
    };
    for (uint32_t bi = 0; bi < r.n_boxes; ++bi) {
        const ffs_box& bx = r.boxes[bi];
        for (int e = 5; e <= 7; ++e) {
            for (long x = (long)bx.l - e; x <= (long)bx.r + e; ++x) { put(x, (long)bx.t - e); put(x, (long)bx.b + e); }
            for (long y = (long)bx.t - e; y <= (long)bx.b + e; ++y) { put((long)bx.l - e, y); put((long)bx.r + e, y); }
        }
    }
    char name[64];
    std::snprintf(name, sizeof name, "pixels_%05u.txt", image_num);
    std::ofstream out(name);
    for (uint32_t y = 0, k = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x, ++k)
            if (r.strong_mask[k]) {
                img[3 * k] = 255; img[3 * k + 1] = 0; img[3 * k + 2] = 0;
                char line[32];
                std::snprintf(line, sizeof line, "%4u, %4u\n", x, y);
                out << line;
            }
    std::snprintf(name, sizeof name, "image_%05u.png", image_num);
    write_png_rgb(name, img.data(), width, height);
}

}  // namespace ffshost
