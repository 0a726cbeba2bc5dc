// Stand-alone driver of the JPEG host stage (yolov4_amd/csrc/jpeg_host.h) for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/jpeg_host_main.cpp -o jpeg_host_main
//   ./jpeg_host_main tests/golden/jpeg
// Every buffer is a heap allocation of exactly the size the entry point is told, so a read past nbytes or a write past coef_cap
// is a report.  Runs the fixtures, every truncation of every fixture, and a deterministic set of single-byte corruptions.
#include <algorithm>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../yolov4_amd/csrc/jpeg_host.h"

namespace {

constexpr long long kCap = 1 << 15;     // coefficient elements offered: a corrupted frame header may ask for far more

struct Outcome {
    int parse, entropy;
};

// the data in a heap block of exactly n bytes; the coefficients in one of exactly min(coef_count, kCap) elements
Outcome run(const unsigned char* src, size_t n) {
    std::unique_ptr<unsigned char[]> data(new unsigned char[n ? n : 1]);
    std::copy(src, src + n, data.get());
    y4_jpeg_info info;
    Outcome o{y4jpeg::parse(data.get(), n, &info), -1};
    if (o.parse != Y4_OK) return o;
    const long long cap = std::min(info.coef_count, kCap);
    std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)cap]);
    std::unique_ptr<uint16_t[]> qt(new uint16_t[3 * 64]);
    o.entropy = y4jpeg::entropy(data.get(), n, &info, coef.get(), cap, qt.get());
    return o;
}

bool known(int code) { return code >= Y4_OK && code <= Y4_ERR_UNSUPPORTED; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <directory of .jpg fixtures>\n", argv[0]);
        return 2;
    }
    std::vector<std::filesystem::path> files;
    for (const auto& e : std::filesystem::directory_iterator(argv[1]))
        if (e.path().extension() == ".jpg") files.push_back(e.path());
    std::sort(files.begin(), files.end());
    if (files.empty()) {
        std::fprintf(stderr, "no fixtures in %s\n", argv[1]);
        return 2;
    }
    long long runs = 0, failures = 0;
    for (const auto& path : files) {
        std::ifstream f(path, std::ios::binary);
        const std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const std::string name = path.filename().string();
        const bool outside = name.rfind("progressive", 0) == 0 || name.rfind("cmyk", 0) == 0;
        const Outcome whole = run(bytes.data(), bytes.size());
        ++runs;
        if (outside ? whole.parse != Y4_ERR_UNSUPPORTED : (whole.parse != Y4_OK || whole.entropy != Y4_OK)) {
            std::fprintf(stderr, "%s: parse %d entropy %d\n", name.c_str(), whole.parse, whole.entropy);
            ++failures;
        }
        for (size_t n = 0; n < bytes.size(); ++n, ++runs) {                 // every truncation
            const Outcome o = run(bytes.data(), n);
            if (!known(o.parse) || (o.parse == Y4_OK && !known(o.entropy))) ++failures;
            if (n + 2 < bytes.size() && o.parse == Y4_OK && o.entropy == Y4_OK) {
                // only the EOI marker may be missing from a file that still decodes
                std::fprintf(stderr, "%s: decodes when cut to %zu of %zu bytes\n", name.c_str(), n, bytes.size());
                ++failures;
            }
        }
        static const unsigned char kFlip[3] = {0xFF, 0x01, 0x80};            // single-byte corruptions
        std::vector<unsigned char> bad(bytes);
        for (size_t p = 0; p < bytes.size(); ++p, ++runs) {
            bad[p] = (unsigned char)(bytes[p] ^ kFlip[p % 3]);
            const Outcome o = run(bad.data(), bad.size());
            if (!known(o.parse) || (o.parse == Y4_OK && !known(o.entropy))) ++failures;
            bad[p] = bytes[p];
        }
    }
    std::printf("%zu fixtures, %lld runs, %lld failures\n", files.size(), runs, failures);
    return failures ? 1 : 0;
}
