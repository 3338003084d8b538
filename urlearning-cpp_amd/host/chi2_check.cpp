// chi2_check -- ulg_chi2_log_sf's routine (csrc/chi2.h) stand-alone, for the
// tests and for a build under the sanitizers (make bin/san/chi2_check):
//
//   chi2_check <dof,dof,...> <x,x,...>
//
// prints one line "dof x value" per grid point, dof outermost, every number as
// "%.17g" (a value reads back to the same double).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/chi2.h"

static bool parse_list(const char *arg, std::vector<double> &out) {
    const std::string s = arg;
    size_t i = 0;
    while (i <= s.size()) {
        const size_t j = std::min(s.find(',', i), s.size());
        const std::string tok = s.substr(i, j - i);
        char *end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (tok.empty() || end != tok.c_str() + tok.size()) return false;
        out.push_back(v);
        i = j + 1;
    }
    return !out.empty();
}

int main(int argc, char **argv) {
    std::vector<double> dofs, xs;
    if (argc != 3 || !parse_list(argv[1], dofs) || !parse_list(argv[2], xs)) {
        std::fprintf(stderr, "usage: chi2_check <dof,dof,...> <x,x,...>\n");
        return 2;
    }
    for (double d : dofs)
        for (double x : xs) std::printf("%.17g %.17g %.17g\n", d, x, ulg::chi2_log_sf(x, d));
    return 0;
}
