// records_dump -- prints what the discrete CSV reader of `score -f BIC`
// (io.cpp load_discrete_csv, the restatement of RecordFile::read,
// base/record_file.h:39-54, and BayesianNetwork::initialize,
// base/variable.h:43-64) makes of a data file:
//   N <records>
//   n <variables>
//   names <name> ...
//   arity <arity> ...
//   then one line per record: its value codes, space separated.
// Used by the CPU tests to check the reader without a GPU.
//
//   records_dump <data.csv> [-s] [-d <delimiter>]
#include <cstdio>
#include <cstring>
#include <string>

#include "io.h"

int main(int argc, char **argv) {
    bool has_header = false;
    char delim = ',';
    std::string pos;
    int npos = 0;
    for (int i = 1; i < argc; ++i) {
        if (std::strcmp(argv[i], "-s") == 0) has_header = true;
        else if (std::strcmp(argv[i], "-d") == 0 && i + 1 < argc && argv[i + 1][0]) delim = argv[++i][0];
        else if (npos < 1) pos = argv[i], ++npos;
        else npos = 2;
    }
    if (npos != 1) {
        std::fprintf(stderr, "usage: records_dump data.csv [-s] [-d <delimiter>]\n");
        return 2;
    }
    ulgio::DiscreteData dd;
    std::string err;
    if (!ulgio::load_discrete_csv(pos, delim, has_header, dd, err)) {
        std::fprintf(stderr, "records_dump: %s\n", err.c_str());
        return 1;
    }
    const size_t n = dd.names.size();
    std::printf("N %lld\nn %zu\nnames", (long long)dd.num_records, n);
    for (const std::string &s : dd.names) std::printf(" %s", s.c_str());
    std::printf("\narity");
    for (int a : dd.arity) std::printf(" %d", a);
    std::printf("\n");
    for (int64_t r = 0; r < dd.num_records; ++r) {
        for (size_t c = 0; c < n; ++c)
            std::printf(c ? " %d" : "%d", (int)dd.codes[c * (size_t)dd.num_records + (size_t)r]);
        std::printf("\n");
    }
    return 0;
}
