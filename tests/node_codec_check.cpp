// Host check of arroy_amd/csrc/node_codec.h (its own main, no device call; built with AddressSanitizer and UBSan by
// tests/test_node_codec_cpu.py).  Reads cases, one per line, and prints the encoded value of each as hex:
//   D <n> <id> ... <id>                                   a Descendants node
//   S <left> <right> <header bytes> <vector bytes> <hex>  a split node; <hex> = [header][vector], or "-" for no normal
// Every value is written into a heap block of exactly the length the size function gives (the sanitizer sees one byte
// more), and the lengths are held against each other: measured = written <= 9 + 10 count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../arroy_amd/csrc/node_codec.h"

namespace codec = ah::codec;

static void print_hex(const std::vector<uint8_t> &v) {
    static const char *digits = "0123456789abcdef";
    std::string s;
    s.reserve(2 * v.size() + 1);
    for (uint8_t b : v) {
        s.push_back(digits[b >> 4]);
        s.push_back(digits[b & 15]);
    }
    std::cout << s << "\n";
}

static int fail(size_t line, const char *what) {
    std::fprintf(stderr, "case %zu: %s\n", line, what);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return fail(0, "usage: node_codec_check CASES");
    std::ifstream in(argv[1]);
    if (!in) return fail(0, "cannot open the cases");
    std::string text;
    size_t line = 0, n_desc = 0, n_split = 0;
    while (std::getline(in, text)) {
        line++;
        if (text.empty() || text[0] == '#') continue;
        std::istringstream ss(text);
        std::string kind;
        ss >> kind;
        if (kind == "D") {
            uint64_t n = 0;
            ss >> n;
            std::vector<uint32_t> ids(n);
            for (uint64_t i = 0; i < n; i++) ss >> ids[i];
            if (!ss) return fail(line, "short id list");
            uint32_t nc = 0;
            uint64_t len = 0;
            if (!codec::measure_descendants(ids.data(), n, &nc, &len)) return fail(line, "ids do not ascend");
            if (len > codec::descendants_value_bound(n)) return fail(line, "value longer than 9 + 10 count");
            if (n == 0 && len != 9) return fail(line, "an empty list is 9 bytes");
            std::vector<uint8_t> out(len);
            const uint64_t wrote = codec::encode_descendants(out.data(), ids.data(), n);
            if (wrote != len) return fail(line, "written length differs from the measured one");
            // an unsorted variant of the same list must be reported
            if (n >= 2) {
                std::vector<uint32_t> bad(ids);
                bad[n - 1] = bad[n - 2];
                if (codec::measure_descendants(bad.data(), n, &nc, &len)) return fail(line, "a repeated id passed the measure");
            }
            print_hex(out);
            n_desc++;
        } else if (kind == "S") {
            uint32_t left = 0, right = 0;
            uint64_t hs = 0, vs = 0;
            std::string hex;
            ss >> left >> right >> hs >> vs >> hex;
            if (!ss) return fail(line, "short split case");
            std::vector<uint8_t> normal;
            const bool has = hex != "-";
            if (has) {
                if (hex.size() != 2 * (hs + vs)) return fail(line, "normal of the wrong length");
                for (size_t i = 0; i < hex.size(); i += 2) normal.push_back((uint8_t)std::strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            }
            const uint64_t len = codec::split_value_len(has, hs, vs);
            if (len != (has ? 9 + hs + vs : 9)) return fail(line, "split length");
            std::vector<uint8_t> out(len);
            const uint64_t wrote = codec::encode_split(out.data(), left, right, has ? normal.data() : nullptr, hs, has ? normal.data() + hs : nullptr, vs);
            if (wrote != len) return fail(line, "written length differs from split_value_len");
            print_hex(out);
            n_split++;
        } else {
            return fail(line, "unknown case kind");
        }
    }
    std::fprintf(stderr, "%zu Descendants and %zu split values encoded\n", n_desc, n_split);
    return 0;
}
