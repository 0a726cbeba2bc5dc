// Stand-alone driver of the JPEG encoder's host stage (yolov4_amd/csrc/jpeg_enc_host.h) for a sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/jpegenc_host_main.cpp -o jpegenc_host_main
//   ./jpegenc_host_main <directory of baseline .jpg files written with the standard tables>
// Each file is taken apart by the decoder's host stage and put together again from its coefficients.  Every buffer is a heap
// allocation of exactly the size the entry point is told, so a write past out_cap or a read outside the coefficients is a
// report: the output buffer is the file's own size (the bytes must come back equal), then every smaller size down to
// size - 40 and a few tiny ones (Y4_ERR_WORKSPACE each time).  Dummy blocks are poisoned first: the encoder must not read them.
#include <algorithm>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../yolov4_amd/csrc/jpeg_enc_host.h"
#include "../yolov4_amd/csrc/jpeg_host.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <directory of .jpg files>\n", argv[0]);
        return 2;
    }
    std::vector<std::filesystem::path> files;
    for (const auto& e : std::filesystem::directory_iterator(argv[1]))
        if (e.path().extension() == ".jpg") files.push_back(e.path());
    std::sort(files.begin(), files.end());
    if (files.empty()) {
        std::fprintf(stderr, "no files in %s\n", argv[1]);
        return 2;
    }
    long long runs = 0, failures = 0;
    for (const auto& path : files) {
        std::ifstream f(path, std::ios::binary);
        const std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const std::string name = path.filename().string();
        y4_jpeg_info info;
        if (y4jpeg::parse(bytes.data(), bytes.size(), &info) != Y4_OK) {
            std::fprintf(stderr, "%s: does not parse\n", name.c_str());
            ++failures;
            continue;
        }
        std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)info.coef_count]);
        std::unique_ptr<uint16_t[]> qt(new uint16_t[3 * 64]);
        if (y4jpeg::entropy(bytes.data(), bytes.size(), &info, coef.get(), info.coef_count, qt.get()) != Y4_OK) {
            std::fprintf(stderr, "%s: entropy decoding fails\n", name.c_str());
            ++failures;
            continue;
        }
        long long at = 0;
        for (int c = 0; c < info.ncomp; ++c) {
            const int rw = y4jpegenc::real_blocks_w(info, c), rh = y4jpegenc::real_blocks_h(info, c);
            for (int by = 0; by < info.blocks_h[c]; ++by)
                for (int bx = 0; bx < info.blocks_w[c]; ++bx, at += 64)
                    if (bx >= rw || by >= rh) std::fill(coef.get() + at, coef.get() + at + 64, (int16_t)0x5A5A);
        }
        const size_t size = bytes.size();
        if (y4jpegenc::bound(&info) < size) {
            std::fprintf(stderr, "%s: bound %zu below the size %zu\n", name.c_str(), y4jpegenc::bound(&info), size);
            ++failures;
        }
        std::vector<size_t> caps = {size, 0, 1, 19, 20, 300, 700};
        for (size_t cut = 1; cut <= 40 && cut < size; ++cut) caps.push_back(size - cut);
        for (const size_t cap : caps) {
            std::unique_ptr<unsigned char[]> out(new unsigned char[cap ? cap : 1]);
            size_t n = 12345;
            const int rc = y4jpegenc::encode(coef.get(), &info, qt.get(), out.get(), cap, &n);
            ++runs;
            if (cap >= size) {
                if (rc != Y4_OK || n != size || !std::equal(bytes.begin(), bytes.end(), out.get())) {
                    std::fprintf(stderr, "%s: code %d, %zu bytes of %zu, or other bytes\n", name.c_str(), rc, n, size);
                    ++failures;
                }
            } else if (rc != Y4_ERR_WORKSPACE || n != 0) {
                std::fprintf(stderr, "%s: cap %zu of %zu gives code %d, %zu bytes\n", name.c_str(), cap, size, rc, n);
                ++failures;
            }
        }
    }
    std::printf("%zu files, %lld runs, %lld failures\n", files.size(), runs, failures);
    return failures ? 1 : 0;
}
