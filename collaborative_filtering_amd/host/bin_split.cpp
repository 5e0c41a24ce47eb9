// split -- a rating file into the TRAIN / VALIDATE files the fitters and rankeval read: repeated
// pairs dropped (the last line stays), the k-core of the bipartite graph, and a per-user hold-out or
// per-user folds, all on the GPU (cf_holdout_split, csrc/cf_split.hip); this file parses and writes.
// Usage: split <file> --out DIR [--name u0] (--holdout K | --ratio NUM/DEN | --folds F)
//              [--by random|time] [--seed S] [--min-train M] [--kcore-user A] [--kcore-item B]
//              [--min-rating T]
//   lines        "user item rating [timestamp]", separated by tabs or blanks (MovieLens u.data)
//   --min-rating lines with a rating below T are dropped before anything else
//   ids          compacted in ascending id order, so a rating set gives the same files in any line order
//   --by random  (default) a user's edges ordered by a hash of (seed, user, item)
//   --by time    needs the fourth field: the latest edges are held out, ties to the smaller item id
//   output       the first three fields of each kept line, tab-joined, in read order:
//                DIR/<name>.train and DIR/<name>.validate, or with --folds F
//                DIR/fold<f>/<name>.train|.validate for f = 0 .. F-1 (fold f is VALIDATE there).
//                An existing non-empty output file is an error.
// The core runs before the hold-out: a TRAIN degree may end below --kcore-user / --kcore-item.
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>

#include "cf_cli.hpp"

namespace {

struct Field {
    const char* b;
    const char* e;
};

bool parse_u64(Field f, uint64_t& v) {
    if (f.b == f.e) return false;
    v = 0;
    for (const char* p = f.b; p < f.e; ++p) {
        if (*p < '0' || *p > '9' || v > (UINT64_MAX - 9) / 10) return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    return true;
}

void make_dir(const std::string& d) {
    if (mkdir(d.c_str(), 0777) != 0 && errno != EEXIST) cfcli::die("mkdir " + d + ": " + std::strerror(errno));
}

void check_new(const std::string& path) {
    struct stat sb;
    if (stat(path.c_str(), &sb) == 0 && sb.st_size > 0) cfcli::die(path + " exists and is not empty");
}

void write_new(const std::string& path, const std::string& text) {
    check_new(path);
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) cfcli::die("cannot write " + path);
    const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
    if (std::fclose(f) != 0 || !ok) cfcli::die("cannot write " + path);
}

uint32_t compact(const std::vector<uint64_t>& raw, std::vector<uint32_t>& out) {   // ascending id order
    std::vector<uint64_t> ids(raw);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    out.resize(raw.size());
    for (size_t i = 0; i < raw.size(); ++i)
        out[i] = (uint32_t)(std::lower_bound(ids.begin(), ids.end(), raw[i]) - ids.begin());
    return (uint32_t)ids.size();
}

}  // namespace

int main(int argc, char** argv) {
    const char* usage =
        "usage: split <file> --out DIR [--name u0] (--holdout K | --ratio NUM/DEN | --folds F) [--by random|time] "
        "[--seed S] [--min-train M] [--kcore-user A] [--kcore-item B] [--min-rating T]";
    if (argc < 2 || argv[1][0] == '-') cfcli::die(usage);
    const std::string path = argv[1], out = cfcli::opt(argc, argv, "out", ""), name = cfcli::opt(argc, argv, "name", "u0");
    const std::string s_hold = cfcli::opt(argc, argv, "holdout", ""), s_ratio = cfcli::opt(argc, argv, "ratio", ""),
                      s_folds = cfcli::opt(argc, argv, "folds", ""), by = cfcli::opt(argc, argv, "by", "random"),
                      s_minr = cfcli::opt(argc, argv, "min-rating", "");
    if (out.empty() || (int)!s_hold.empty() + (int)!s_ratio.empty() + (int)!s_folds.empty() != 1) cfcli::die(usage);
    if (by != "random" && by != "time") cfcli::die("--by is random or time");
    const auto number = [&](const std::string& flag, const std::string& s) {
        uint64_t v = 0;
        if (!parse_u64(Field{s.data(), s.data() + s.size()}, v)) cfcli::die("--" + flag + " needs a non-negative integer");
        return v;
    };
    const auto number32 = [&](const std::string& flag, const std::string& s) {
        const uint64_t v = number(flag, s);
        if (v > UINT32_MAX) cfcli::die("--" + flag + " is too large");
        return (uint32_t)v;
    };
    int mode = CF_SPLIT_LEAVE_K;
    uint32_t a = 0, b = 0;
    if (!s_hold.empty()) {
        a = number32("holdout", s_hold);
    } else if (!s_ratio.empty()) {
        mode = CF_SPLIT_RATIO;
        const size_t slash = s_ratio.find('/');
        if (slash == std::string::npos) cfcli::die("--ratio needs NUM/DEN");
        a = number32("ratio", s_ratio.substr(0, slash));
        b = number32("ratio", s_ratio.substr(slash + 1));
        if (a == 0 || a >= b) cfcli::die("--ratio needs 0 < NUM < DEN");
    } else {
        mode = CF_SPLIT_FOLDS;
        a = number32("folds", s_folds);
        if (a < 2 || a > 254) cfcli::die("--folds needs 2 .. 254");
    }
    const uint64_t seed = number("seed", cfcli::opt(argc, argv, "seed", "0"));
    const uint32_t min_train = number32("min-train", cfcli::opt(argc, argv, "min-train", "0"));
    const uint32_t min_user = number32("kcore-user", cfcli::opt(argc, argv, "kcore-user", "0"));
    const uint32_t min_item = number32("kcore-item", cfcli::opt(argc, argv, "kcore-item", "0"));
    double min_rating = 0.0;
    if (!s_minr.empty()) {
        const char* p = s_minr.data();
        if (!cfio::parse_f64(p, p + s_minr.size(), min_rating) || p != s_minr.data() + s_minr.size())
            cfcli::die("--min-rating needs a number");
    }

    const uint32_t n_sets = mode == CF_SPLIT_FOLDS ? a : 1;
    const auto set_dir = [&](uint32_t f) { return mode == CF_SPLIT_FOLDS ? out + "/fold" + std::to_string(f) : out; };
    for (uint32_t f = 0; f < n_sets; ++f)   // before any work: nothing is written beside an earlier split
        for (const char* suffix : {".train", ".validate"}) check_new(set_dir(f) + "/" + name + suffix);

    const std::string text = cfio::read_file(path);
    std::vector<uint64_t> raw_user, raw_item, key;
    std::vector<std::string> line3;   // the first three fields of a kept line, tab-joined
    const char* p = text.data();
    const char* end = p + text.size();
    uint64_t lineno = 0, n_lines = 0;
    while (p < end) {
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', end - p));
        const char* le = nl ? nl : end;
        ++lineno;
        Field f[4];
        int nf = 0;
        const char* q = p;
        while (nf < 4) {
            while (q < le && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
            if (q == le) break;
            f[nf].b = q;
            while (q < le && *q != ' ' && *q != '\t' && *q != '\r') ++q;
            f[nf++].e = q;
        }
        p = nl ? nl + 1 : end;
        if (nf == 0) continue;   // an empty line
        const std::string where = path + ":" + std::to_string(lineno);
        uint64_t u = 0, m = 0, t = 0;
        double r = 0.0;
        const char* rb = nf >= 3 ? f[2].b : nullptr;
        if (nf < 3 || !parse_u64(f[0], u) || !parse_u64(f[1], m) || !cfio::parse_f64(rb, f[2].e, r) || rb != f[2].e)
            cfcli::die(where + ": not \"user item rating [timestamp]\"");
        ++n_lines;
        if (!s_minr.empty() && r < min_rating) continue;
        if (by == "time") {
            if (nf < 4 || !parse_u64(f[3], t)) cfcli::die(where + ": --by time needs an integer timestamp in the fourth field");
            key.push_back(UINT64_MAX - t);
        }
        raw_user.push_back(u);
        raw_item.push_back(m);
        std::string s(f[0].b, f[0].e);
        s += '\t';
        s.append(f[1].b, f[1].e);
        s += '\t';
        s.append(f[2].b, f[2].e);
        s += '\n';
        line3.push_back(std::move(s));
    }
    const uint64_t n = raw_user.size();
    std::vector<uint32_t> user, item;
    const uint32_t n_users = compact(raw_user, user), n_items = compact(raw_item, item);

    std::vector<uint8_t> part(std::max<uint64_t>(n, 1));
    uint64_t stats[CF_SPLIT_STATS] = {};
    cf_ctx* ctx = cfcli::open_device();
    cfcli::check(ctx,
                 cf_holdout_split(ctx, n, n_users, n_items, user.data(), item.data(), by == "time" ? key.data() : nullptr,
                                  seed, min_user, min_item, mode, a, b, min_train, part.data(), stats),
                 "cf_holdout_split");
    cf_destroy(ctx);

    make_dir(out);
    for (uint32_t f = 0; f < n_sets; ++f) {
        const std::string dir = set_dir(f);
        if (mode == CF_SPLIT_FOLDS) make_dir(dir);
        const uint8_t held = mode == CF_SPLIT_FOLDS ? (uint8_t)f : (uint8_t)1;
        std::string train, validate;
        for (uint64_t i = 0; i < n; ++i) {
            if (part[i] == CF_SPLIT_DROPPED) continue;
            (part[i] == held ? validate : train) += line3[i];
        }
        write_new(dir + "/" + name + ".train", train);
        write_new(dir + "/" + name + ".validate", validate);
    }
    std::printf("split: lines %llu read %llu kept %llu alive %llu users %llu items %llu train %llu validate %llu "
                "items_without_train %llu rounds %llu\n",
                (unsigned long long)n_lines, (unsigned long long)n, (unsigned long long)stats[0],
                (unsigned long long)stats[1], (unsigned long long)stats[2], (unsigned long long)stats[3],
                (unsigned long long)stats[4], (unsigned long long)stats[5], (unsigned long long)stats[6],
                (unsigned long long)stats[7]);
    return 0;
}
