/*
 * exr.cpp -- OpenEXR writer/reader for developed films (float32, uncompressed
 * scanlines, channels Y or R,G,B[,A]) and for interleaved float32 channels with caller-given names
 * (guide buffers: Z, N.X, ..., id, view).  Replaces the reference's Bitmap/OpenEXR path
 * used by Film::write (src/films/hdrfilm.cpp:420-546, OpenEXR submodule not vendored).
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/amvpt_host.h"

void amvpt_host_set_error(const std::string &msg);

namespace {
void put_bytes(std::vector<uint8_t> &b, const void *p, size_t n) {
    const uint8_t *c = (const uint8_t *) p;
    b.insert(b.end(), c, c + n);
}
void put_i32(std::vector<uint8_t> &b, int32_t v) { put_bytes(b, &v, 4); }
void put_str(std::vector<uint8_t> &b, const char *s) { put_bytes(b, s, std::strlen(s) + 1); }
void attr(std::vector<uint8_t> &b, const char *name, const char *type, const std::vector<uint8_t> &v) {
    put_str(b, name);
    put_str(b, type);
    put_i32(b, (int32_t) v.size());
    b.insert(b.end(), v.begin(), v.end());
}
const char *const kNames1[] = {"Y"};
const char *const kNames3[] = {"R", "G", "B"};
const char *const kNames4[] = {"R", "G", "B", "A"};
int fail(const std::string &msg) {
    amvpt_host_set_error(msg);
    return -1;
}

/* the caller's channel names: 1 to 31 bytes (the format's limit) and unique; order[k] = the source channel of the
 * k-th channel in the byte order of the names, the order the format stores them in */
int check_names(const char *who, uint32_t c, const char *const *names, std::vector<uint32_t> &order) {
    const std::string w = std::string(who) + ": ";
    if (c == 0) return fail(w + "no channels");
    if (!names) return fail(w + "null names");
    for (uint32_t k = 0; k < c; ++k) {
        if (!names[k]) return fail(w + "channel " + std::to_string(k) + " has a null name");
        const size_t len = std::strlen(names[k]);
        if (len == 0) return fail(w + "channel " + std::to_string(k) + " has an empty name");
        if (len > 31) return fail(w + "channel " + std::to_string(k) + " (\"" + names[k] + "\") has a name longer than 31 bytes");
        for (uint32_t j = 0; j < k; ++j)
            if (std::strcmp(names[j], names[k]) == 0)
                return fail(w + "channel " + std::to_string(k) + " repeats the name \"" + names[k] + "\" of channel " + std::to_string(j));
    }
    order.resize(c);
    for (uint32_t k = 0; k < c; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return std::strcmp(names[a], names[b]) < 0; });
    return 0;
}

int write_channels(const char *who, const char *path, const float *data, uint32_t w, uint32_t h, uint32_t c,
                   const char *const *names) {
    std::vector<uint32_t> order;
    if (int rc = check_names(who, c, names, order)) return rc;
    if (!path || !data) return fail(std::string(who) + ": null argument");
    if (!w || !h) return fail(std::string(who) + ": empty image");
    std::vector<uint8_t> b;
    put_i32(b, 20000630);
    put_i32(b, 2);
    std::vector<uint8_t> v;
    for (uint32_t k = 0; k < c; ++k) {
        put_str(v, names[order[k]]);
        put_i32(v, 2);                 /* FLOAT */
        uint8_t lin[4] = {0, 0, 0, 0}; /* pLinear + reserved */
        put_bytes(v, lin, 4);
        put_i32(v, 1);
        put_i32(v, 1);
    }
    v.push_back(0);
    attr(b, "channels", "chlist", v);
    attr(b, "compression", "compression", std::vector<uint8_t>{0});
    v.clear();
    put_i32(v, 0); put_i32(v, 0); put_i32(v, (int32_t) w - 1); put_i32(v, (int32_t) h - 1);
    attr(b, "dataWindow", "box2i", v);
    attr(b, "displayWindow", "box2i", v);
    attr(b, "lineOrder", "lineOrder", std::vector<uint8_t>{0});
    v.clear();
    float one = 1.f, zero[2] = {0.f, 0.f};
    put_bytes(v, &one, 4);
    attr(b, "pixelAspectRatio", "float", v);
    v.clear();
    put_bytes(v, zero, 8);
    attr(b, "screenWindowCenter", "v2f", v);
    v.clear();
    put_bytes(v, &one, 4);
    attr(b, "screenWindowWidth", "float", v);
    b.push_back(0);
    const size_t line_bytes = (size_t) w * c * 4;
    uint64_t off = b.size() + 8ull * h;
    for (uint32_t y = 0; y < h; ++y) {
        put_bytes(b, &off, 8);
        off += 8 + line_bytes;
    }
    std::vector<float> line((size_t) w * c);
    for (uint32_t y = 0; y < h; ++y) {
        put_i32(b, (int32_t) y);
        put_i32(b, (int32_t) line_bytes);
        for (uint32_t k = 0; k < c; ++k) {
            const uint32_t src = order[k];
            for (uint32_t x = 0; x < w; ++x) line[(size_t) k * w + x] = data[((size_t) y * w + x) * c + src];
        }
        put_bytes(b, line.data(), line_bytes);
    }
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(std::string(who) + ": cannot open " + path);
    size_t n = std::fwrite(b.data(), 1, b.size(), f);
    std::fclose(f);
    return n == b.size() ? 0 : fail(std::string(who) + ": short write to " + path);
}

/* Reads files produced by write_channels (same layout): every named channel must be one of the file's float32
 * channels, whose count must be c */
int read_channels(const char *who, const char *path, float *data, uint32_t w, uint32_t h, uint32_t c,
                  const char *const *names) {
    const std::string wh = std::string(who) + ": ";
    std::vector<uint32_t> order;
    if (int rc = check_names(who, c, names, order)) return rc;
    if (!path || !data) return fail(wh + "null argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(wh + "cannot open " + path);
    std::vector<uint8_t> b;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    std::fclose(f);
    if (b.size() < 8) return fail(wh + "truncated file");
    int32_t magic;
    std::memcpy(&magic, b.data(), 4);
    if (magic != 20000630) return fail(wh + "not an OpenEXR file");
    b.push_back(0);   /* a terminator for the header's strings, whatever the file holds */
    const size_t end = b.size() - 1;
    std::vector<std::string> file_names;
    bool have_list = false;
    size_t p = 8;
    while (p < end && b[p] != 0) {
        std::string name((const char *) &b[p]);
        p += name.size() + 1;
        if (p >= end) return fail(wh + "truncated header");
        std::string type((const char *) &b[p]);
        p += type.size() + 1;
        if (p + 4 > end) return fail(wh + "truncated header");
        int32_t sz;
        std::memcpy(&sz, &b[p], 4);
        p += 4;
        if (sz < 0 || p + (size_t) sz > end) return fail(wh + "truncated header");
        if (name == "channels") {
            have_list = true;
            size_t q = p;
            const size_t qe = p + (size_t) sz;
            while (q < qe && b[q] != 0) {
                std::string ch((const char *) &b[q]);
                q += ch.size() + 1;
                if (q + 16 > qe) return fail(wh + "truncated channel list");
                int32_t pixel_type;
                std::memcpy(&pixel_type, &b[q], 4);
                if (pixel_type != 2) return fail(wh + "channel \"" + ch + "\" is not float32");
                q += 16;
                file_names.push_back(ch);
            }
        }
        p += (size_t) sz;
    }
    if (!have_list) return fail(wh + "no channel list");
    if (file_names.size() != c)
        return fail(wh + "the file holds " + std::to_string(file_names.size()) + " channels, not " + std::to_string(c));
    /* the file's k-th channel -> the caller's channel of that name */
    std::vector<uint32_t> dst(c);
    for (uint32_t k = 0; k < c; ++k) {
        uint32_t j = 0;
        while (j < c && file_names[k] != names[j]) ++j;
        if (j == c) return fail(wh + "the file's channel \"" + file_names[k] + "\" is not among the names asked for");
        dst[k] = j;
    }
    p += 1 + 8ull * h;
    const size_t line_bytes = (size_t) w * c * 4;
    for (uint32_t y = 0; y < h; ++y) {
        if (p + 8 + line_bytes > end) return fail(wh + "truncated scanline data");
        p += 8;
        for (uint32_t k = 0; k < c; ++k)
            for (uint32_t x = 0; x < w; ++x)
                std::memcpy(&data[((size_t) y * w + x) * c + dst[k]], &b[p + ((size_t) k * w + x) * 4], 4);
        p += line_bytes;
    }
    return 0;
}
const char *const *rgb_names(uint32_t c) { return c == 1 ? kNames1 : c == 3 ? kNames3 : kNames4; }
} // namespace

extern "C" int amvpt_host_write_exr(const char *path, const float *data, uint32_t w, uint32_t h, uint32_t c) {
    if (c != 1 && c != 3 && c != 4) return fail("write_exr: channel count must be 1, 3 or 4");
    return write_channels("write_exr", path, data, w, h, c, rgb_names(c));
}

/* Reads files produced by amvpt_host_write_exr (same layout). */
extern "C" int amvpt_host_read_exr(const char *path, float *data, uint32_t w, uint32_t h, uint32_t c) {
    if (c != 1 && c != 3 && c != 4) return fail("read_exr: channel count must be 1, 3 or 4");
    return read_channels("read_exr", path, data, w, h, c, rgb_names(c));
}

extern "C" int amvpt_host_write_exr_channels(const char *path, const float *data, uint32_t w, uint32_t h, uint32_t c,
                                             const char *const *names) {
    return write_channels("write_exr_channels", path, data, w, h, c, names);
}

extern "C" int amvpt_host_read_exr_channels(const char *path, float *data, uint32_t w, uint32_t h, uint32_t c,
                                            const char *const *names) {
    return read_channels("read_exr_channels", path, data, w, h, c, names);
}
