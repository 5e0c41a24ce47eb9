// cf_factor_io.hpp -- reader of the factor files the matrix-factorization binaries write
// (cf_mf_cli.hpp write_vertex_values): shards "<P>.U_<i>_of_<n>" / "<P>.V_<i>_of_<n>" with one line
// per vertex, "id f0 f1 .. " or "id) f0 f1 .. " (both spellings occur: als.cpp:521-525 and
// :542-546, sgd.cpp:435,456), 17 significant digits per value, which parse back to the same
// doubles; the bias files "<P>.bias.U_*" / "<P>.bias.V_*" are the same lines with one value.
#pragma once

#include <charconv>
#include <string>
#include <vector>

#include "cf_cli.hpp"

namespace cfmf {

struct Factors {
    cfio::IdMap ids;         // ascending ids -> row
    uint32_t width = 0;      // values per line (D, or 1 for a bias file)
    std::vector<double> F;   // ids.size() x width, row-major
};

// Every shard of `prefix` + "_" (prefix may hold a directory part).  The width is the first
// line's; a line of another width, a line that does not parse and an id given twice are fatal.
inline Factors read_factors(const std::string& prefix) {
    const size_t slash = prefix.rfind('/');
    const std::string dir = slash == std::string::npos ? std::string(".") : prefix.substr(0, slash + 1);
    const std::string base = (slash == std::string::npos ? prefix : prefix.substr(slash + 1)) + "_";
    const std::vector<std::string> files = cfio::files_with_prefix(dir, base);
    if (files.empty()) cfcli::die("no factor file " + prefix + "_*");
    std::vector<uint32_t> id_of_line;
    std::vector<double> vals;
    Factors f;
    for (const std::string& path : files) {
        const std::string text = cfio::read_file(path);
        size_t pos = 0, line_no = 0;
        while (pos < text.size()) {
            size_t nl = text.find('\n', pos);
            if (nl == std::string::npos) nl = text.size();
            const char* p = text.data() + pos;
            const char* e = text.data() + nl;
            pos = nl + 1;
            ++line_no;
            const auto skip = [&] {
                while (p < e && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
            };
            skip();
            if (p == e) continue;
            const std::string where = path + " line " + std::to_string(line_no);
            uint32_t id = 0;
            const auto r = std::from_chars(p, e, id);
            if (r.ec != std::errc()) cfcli::die("factor line without an id: " + where);
            p = r.ptr;
            if (p < e && *p == ')') ++p;
            uint32_t w = 0;
            for (skip(); p < e; skip()) {
                double v;
                if (!cfio::parse_f64(p, e, v)) cfcli::die("factor line with a value that does not parse: " + where);
                vals.push_back(v);
                ++w;
            }
            if (id_of_line.empty()) f.width = w;
            if (w != f.width || w == 0)
                cfcli::die("factor line of another width: " + where + " holds " + std::to_string(w) + " values, the first line " +
                           std::to_string(f.width));
            id_of_line.push_back(id);
        }
    }
    if (id_of_line.empty()) cfcli::die("no factor line in " + prefix + "_*");
    f.ids.build(id_of_line);
    if (f.ids.size() != id_of_line.size()) cfcli::die("an id appears twice in " + prefix + "_*");
    f.F.resize((size_t)f.ids.size() * f.width);
    for (size_t l = 0; l < id_of_line.size(); ++l) {
        const uint32_t row = f.ids.at[id_of_line[l]];
        for (uint32_t d = 0; d < f.width; ++d) f.F[(size_t)row * f.width + d] = vals[l * f.width + d];
    }
    return f;
}

// A bias file of the vertices of `like`: one value per id, every id of `like` present.
inline std::vector<double> read_bias(const std::string& prefix, const Factors& like) {
    const Factors b = read_factors(prefix);
    if (b.width != 1) cfcli::die("bias file " + prefix + "_* holds " + std::to_string(b.width) + " values per line");
    std::vector<double> out(like.ids.size(), 0.0);
    for (uint32_t i = 0; i < like.ids.size(); ++i) {
        const auto it = b.ids.at.find(like.ids.ids[i]);
        if (it == b.ids.at.end()) cfcli::die("id " + std::to_string(like.ids.ids[i]) + " has no line in " + prefix + "_*");
        out[i] = b.F[it->second];
    }
    return out;
}

}  // namespace cfmf
