// Stand-alone host program of the spring builder (csrc/springs.hpp; no HIP, plain g++). Reads
// cases from argv[1], each "<name> <n verts> <n springs> <mode> <flags>" followed by the vertices
// (3 numbers each), the pairs (2 indices each), k and rest (n numbers each; nan / inf accepted).
// flags: 1 = pass the vertices (else NULL), 2 = pass rest (else NULL), 4 = pass pairs as NULL,
// 8 = pass k as NULL. Prints per case
//   set <name> <n springs>
//   s <a> <b> <G0> <G1> <L> <w>        (one line per spring, %.17g)
// or, for a refused case,
//   error <name> <code> <message>
// tests/test_springs.py compares the lines with the numpy restatement (tests/spring_cases.py).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "springs.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: springs cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::string name, tok;
    int n_cases = 0;
    while (in >> name) {
        int nv = 0, n = 0, mode = 0, flags = 0;
        if (!(in >> nv >> n >> mode >> flags)) { std::printf("bad header of %s\n", name.c_str()); return 2; }
        const int m = n > 0 ? n : 0;
        std::vector<double> V(3 * (size_t)nv), k(m), rest(m);
        std::vector<int> P(2 * (size_t)m);
        for (auto& c : V) { if (!(in >> tok)) return 2; c = std::strtod(tok.c_str(), nullptr); }
        for (auto& i : P) if (!(in >> i)) return 2;
        for (auto& c : k) { if (!(in >> tok)) return 2; c = std::strtod(tok.c_str(), nullptr); }
        for (auto& c : rest) { if (!(in >> tok)) return 2; c = std::strtod(tok.c_str(), nullptr); }
        try {
            const aa::SpringSet S = aa::build_springs((flags & 1) ? V.data() : nullptr, nv, (flags & 4) ? nullptr : P.data(), n, mode,
                                                      (flags & 8) ? nullptr : k.data(), (flags & 2) ? rest.data() : nullptr);
            std::printf("set %s %d\n", name.c_str(), S.count());
            for (int e = 0; e < S.count(); ++e)
                std::printf("s %d %d %.17g %.17g %.17g %.17g\n", S.idx[2 * e], S.idx[2 * e + 1], S.G[2 * e], S.G[2 * e + 1], S.L[e], S.w[e]);
        } catch (const aa::Error& err) {
            std::printf("error %s %d %s\n", name.c_str(), err.code, err.what());
        }
        ++n_cases;
    }
    std::printf("ok %d cases\n", n_cases);
    return 0;
}
