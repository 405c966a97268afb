/*
 * display.cpp -- the files of the display stage: the reference's presets.csv (src/mitsuba/preset.h:19-107) and an
 * 8-bit RGB PNG writer for the quilt and the interlaced image (the reference writes them through Bitmap::write and
 * libpng, program.h:60, program.cpp:270-271).  The PNG holds stored (uncompressed) deflate blocks, with CRC-32 and
 * Adler-32 computed here: no compression library is linked.
 */
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/amvpt_host.h"

void amvpt_host_set_error(const std::string &msg);

namespace {
int fail(const std::string &msg) {
    amvpt_host_set_error(msg);
    return -1;
}

uint32_t crc32_of(const uint8_t *p, size_t n, uint32_t crc = 0) {
    /* built once, by the first caller (initialisation of a local static is thread-safe) */
    static const std::array<uint32_t, 256> table = [] {
        std::array<uint32_t, 256> t{};
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

void put_be32(std::vector<uint8_t> &b, uint32_t v) {
    for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t) (v >> s));
}

/* length, type, data, CRC-32 over type + data */
void put_chunk(std::vector<uint8_t> &png, const char *type, const std::vector<uint8_t> &data) {
    put_be32(png, (uint32_t) data.size());
    const size_t at = png.size();
    png.insert(png.end(), type, type + 4);
    png.insert(png.end(), data.begin(), data.end());
    put_be32(png, crc32_of(png.data() + at, png.size() - at));
}

/* one field of a presets.csv line; false when the line has run out */
bool next_field(const std::string &line, size_t &pos, std::string &out) {
    if (pos > line.size()) return false;
    const size_t end = line.find(';', pos);
    out = line.substr(pos, end == std::string::npos ? std::string::npos : end - pos);
    pos = end == std::string::npos ? line.size() + 1 : end + 1;
    return true;
}
} // namespace

extern "C" int amvpt_host_write_png(const char *path, const uint8_t *rgb, uint32_t w, uint32_t h) {
    if (!path || !rgb) return fail("write_png: null argument");
    if (!w || !h) return fail("write_png: empty image");
    const size_t row = (size_t) w * 3;
    if (row + 1 > 0x7fffffffu / h) return fail("write_png: image too large for one IDAT chunk");
    /* the filtered image: filter type 0 (None) before every row */
    std::vector<uint8_t> raw;
    raw.reserve((row + 1) * h);
    for (uint32_t y = 0; y < h; ++y) {
        raw.push_back(0);
        raw.insert(raw.end(), rgb + y * row, rgb + (y + 1) * row);
    }
    /* zlib stream: header, stored blocks of at most 65535 bytes, Adler-32 of the raw bytes */
    std::vector<uint8_t> z;
    z.reserve(raw.size() + raw.size() / 65535 * 5 + 16);
    z.push_back(0x78);
    z.push_back(0x01);
    uint32_t a = 1, b = 0;
    for (size_t at = 0; at < raw.size();) {
        const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
        z.push_back(at + n == raw.size() ? 1 : 0);   /* BFINAL, BTYPE = 00 */
        z.push_back((uint8_t) (n & 0xff));
        z.push_back((uint8_t) (n >> 8));
        z.push_back((uint8_t) (~n & 0xff));
        z.push_back((uint8_t) ((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + n);
        for (size_t i = at; i < at + n; ++i) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
        at += n;
    }
    put_be32(z, (b << 16) | a);

    std::vector<uint8_t> png = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, w);
    put_be32(ihdr, h);
    const uint8_t tail[5] = {8, 2, 0, 0, 0};   /* bit depth 8, colour type 2 (RGB), deflate, adaptive, no interlace */
    ihdr.insert(ihdr.end(), tail, tail + 5);
    put_chunk(png, "IHDR", ihdr);
    put_chunk(png, "IDAT", z);
    put_chunk(png, "IEND", {});
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(std::string("write_png: cannot open ") + path);
    const bool ok = std::fwrite(png.data(), 1, png.size(), f) == png.size();
    if (std::fclose(f) != 0 || !ok) return fail(std::string("write_png: short write to ") + path);
    return 0;
}

extern "C" int amvpt_host_write_presets(const char *path, const amvpt_host_named_preset *presets, uint32_t count) {
    if (!path || (count && !presets)) return fail("write_presets: null argument");
    FILE *f = std::fopen(path, "w");
    if (!f) return fail(std::string("Error opening file for writing: ") + path);
    for (uint32_t i = 0; i < count; ++i) {
        const amvpt_display_preset &p = presets[i].preset;
        char name[65];
        std::memcpy(name, presets[i].name, 64);
        name[64] = 0;
        if (std::strpbrk(name, ";\n")) {
            std::fclose(f);
            return fail("write_presets: a preset name holds ';' or a line break");
        }
        std::fprintf(f, "%s;%.9g;%.9g;%.9g;%.9g;%.9g;%.9g;%.9g;%d;%d;%u\n", name, (double) p.center, (double) p.focus,
                     (double) p.pitch, (double) p.tilt, (double) p.subp, (double) p.view[0], (double) p.view[1],
                     (int) p.grid[0], (int) p.grid[1], p.flip_rgb ? 1u : 0u);
    }
    if (std::fclose(f) != 0) return fail(std::string("write_presets: short write to ") + path);
    return 0;
}

extern "C" int amvpt_host_read_presets(const char *path, amvpt_host_named_preset *presets, uint32_t capacity,
                                       uint32_t *count) {
    if (!path || !count || (capacity && !presets)) return fail("read_presets: null argument");
    std::ifstream file(path);
    if (!file) return fail(std::string("Error opening file for reading: ") + path);
    std::string line;
    uint32_t n = 0, lineno = 0;
    while (std::getline(file, line)) {
        ++lineno;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        size_t pos = 0;
        std::string field[11];
        for (int k = 0; k < 11; ++k)
            if (!next_field(line, pos, field[k]))
                return fail("read_presets: line " + std::to_string(lineno) + " of " + path + " has " + std::to_string(k) +
                            " fields, not 11");
        amvpt_host_named_preset e;
        std::memset(&e, 0, sizeof(e));
        std::strncpy(e.name, field[0].c_str(), 63);
        float *fv[7] = {&e.preset.center, &e.preset.focus, &e.preset.pitch, &e.preset.tilt, &e.preset.subp,
                        &e.preset.view[0], &e.preset.view[1]};
        for (int k = 0; k < 10; ++k) {
            const char *s = field[k + 1].c_str();
            char *end = nullptr;
            if (k < 7) *fv[k] = std::strtof(s, &end);
            else if (k < 9) e.preset.grid[k - 7] = (int32_t) std::strtol(s, &end, 10);
            else e.preset.flip_rgb = std::strtol(s, &end, 10) ? 1u : 0u;
            if (end == s)
                return fail("read_presets: line " + std::to_string(lineno) + " of " + path + ": field " +
                            std::to_string(k + 2) + " is not a number");
        }
        if (n < capacity) presets[n] = e;
        ++n;
    }
    *count = n;
    return 0;
}
