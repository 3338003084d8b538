// constraints_dump -- prints what the drop-in constraints reader (io.cpp
// read_constraints, the restatement of scoring::parseConstraints,
// scoring_function/constraints.h:161-236) parses, against the variable names
// the score command takes from the same CSV (record_stats):
//   <variable> <required parents as u64> <forbidden parents as u64>
// one line per alternative, in file order.  Used by the CPU tests to check
// the parser without a GPU.
//
//   constraints_dump <constraints> <data.csv> [-s] [-d <delimiter>]
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "io.h"

int main(int argc, char **argv) {
    bool has_header = false;
    char delim = ',';
    std::string pos[2];
    int npos = 0;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "-s") == 0) has_header = true;
        else if (std::strcmp(argv[i], "-d") == 0 && i + 1 < argc && argv[i + 1][0]) delim = argv[++i][0];
        else if (npos < 2) pos[npos++] = argv[i];
        else npos = 3;
    }
    if (npos != 2) {
        std::fprintf(stderr, "usage: constraints_dump constraints.txt data.csv [-s] [-d <delimiter>]\n");
        return 2;
    }
    ulgio::RecordStats rs;
    if (!ulgio::record_stats(pos[1], delim, has_header, rs)) {
        std::fprintf(stderr, "constraints_dump: cannot read '%s'\n", pos[1].c_str());
        return 1;
    }
    ulgio::Constraints cons;
    std::string err;
    if (!ulgio::read_constraints(pos[0], rs.names, cons, err)) {
        std::fprintf(stderr, "constraints_dump: %s\n", err.c_str());
        return 1;
    }
    for (size_t i = 0; i < cons.vars.size(); ++i)
        std::printf("%d %" PRIu64 " %" PRIu64 "\n", cons.vars[i], cons.required[i], cons.forbidden[i]);
    return 0;
}
