// Stand-alone host program of the tie builder (csrc/ties.hpp; no HIP, plain g++). Reads cases from
// argv[1], each "<name> <n verts> <n ties> <na> <nb> <mode> <flags>" followed by the vertices (3
// numbers each), nodes_a (na indices per tie), w_a (na numbers per tie), nodes_b, w_b (nb per tie), k
// and rest (n numbers each; nan / inf accepted). flags: 1 = pass the vertices (else NULL), 2 = pass
// rest (else NULL), 4 = pass nodes_a as NULL, 8 = pass k as NULL, 16 = pass w_b as NULL. Prints per case
//   set <name> <n ties> <nv>
//   t <idx x nv> <G x nv> <L> <w>        (one line per tie, %.17g)
// or, for a refused case,
//   error <name> <code> <message>
// tests/test_ties.py compares the lines with the numpy restatement (tests/tie_cases.py).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "ties.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: ties cases.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::string name, tok;
    int n_cases = 0;
    while (in >> name) {
        int nv = 0, n = 0, na = 0, nb = 0, mode = 0, flags = 0;
        if (!(in >> nv >> n >> na >> nb >> mode >> flags)) { std::printf("bad header of %s\n", name.c_str()); return 2; }
        const size_t m = n > 0 ? n : 0, ca = na > 0 ? na : 0, cb = nb > 0 ? nb : 0;
        std::vector<double> V(3 * (size_t)nv), wa(m * ca), wb(m * cb), k(m), rest(m);
        std::vector<int> A(m * ca), B(m * cb);
        auto num = [&](double& c) { if (!(in >> tok)) return false; c = std::strtod(tok.c_str(), nullptr); return true; };
        for (auto& c : V) if (!num(c)) return 2;
        for (auto& i : A) if (!(in >> i)) return 2;
        for (auto& c : wa) if (!num(c)) return 2;
        for (auto& i : B) if (!(in >> i)) return 2;
        for (auto& c : wb) if (!num(c)) return 2;
        for (auto& c : k) if (!num(c)) return 2;
        for (auto& c : rest) if (!num(c)) return 2;
        try {
            const aa::TieSet S = aa::build_ties((flags & 1) ? V.data() : nullptr, nv, na, (flags & 4) ? nullptr : A.data(), wa.data(), nb,
                                                B.data(), (flags & 16) ? nullptr : wb.data(), n, mode, (flags & 8) ? nullptr : k.data(),
                                                (flags & 2) ? rest.data() : nullptr);
            std::printf("set %s %d %d\n", name.c_str(), S.count(), S.nv);
            for (int e = 0; e < S.count(); ++e) {
                std::printf("t");
                for (int a = 0; a < S.nv; ++a) std::printf(" %d", S.idx[(size_t)S.nv * e + a]);
                for (int a = 0; a < S.nv; ++a) std::printf(" %.17g", S.G[(size_t)S.nv * e + a]);
                std::printf(" %.17g %.17g\n", S.L[e], S.w[e]);
            }
        } catch (const aa::Error& err) {
            std::printf("error %s %d %s\n", name.c_str(), err.code, err.what());
        }
        ++n_cases;
    }
    std::printf("ok %d cases\n", n_cases);
    return 0;
}
