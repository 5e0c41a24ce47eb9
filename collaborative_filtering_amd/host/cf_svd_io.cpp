// cf_svd_io.cpp -- see cf_svd_io.hpp.
#include "cf_svd_io.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "cf_mf_cli.hpp"

namespace cfsvdio {

namespace {

bool ends_with(const std::string& s, const std::string& suffix) {
    return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

std::string base_name(const std::string& path) {
    const size_t p = path.find_last_of('/');
    return p == std::string::npos ? path : path.substr(p + 1);
}

}  // namespace

Matrix load_matrix(const std::string& dir, const std::string& vecfile, uint32_t rows, uint32_t cols) {
    Matrix m;
    const std::string vec_base = base_name(vecfile);
    for (const std::string& path : cfio::files_with_suffix(dir, "")) {
        if (!vecfile.empty() && (path == vecfile || base_name(path) == vec_base)) continue;
        if (ends_with(path, "singular_values") || ends_with(path, "_v0")) continue;
        const std::string text = cfio::read_file(path);
        const char* p = text.c_str();
        const char* end = p + text.size();
        while (p < end) {
            const char* eol = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
            if (!eol) eol = end;
            const std::string line(p, eol);
            p = eol + 1;
            if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
            char* q = nullptr;
            const char* s = line.c_str();
            const unsigned long long r = std::strtoull(s, &q, 10);
            if (q == s) throw std::runtime_error("cannot parse a line of " + path + ": " + line);
            s = q;
            const unsigned long long c = std::strtoull(s, &q, 10);
            if (q == s) throw std::runtime_error("cannot parse a line of " + path + ": " + line);
            const float v = std::strtof(q, nullptr);   // a missing value reads as 0, as `strm >> obs` leaves it
            if (r < 1 || r > rows)
                throw std::runtime_error("row id " + std::to_string(r) + " outside 1.." + std::to_string(rows) + " in " + path);
            if (c < 1 || c > cols)
                throw std::runtime_error("column id " + std::to_string(c) + " outside 1.." + std::to_string(cols) + " in " + path);
            m.row.push_back((uint32_t)(r - 1));
            m.col.push_back((uint32_t)(c - 1));
            m.val.push_back(v);
        }
    }
    return m;
}

std::vector<double> load_initial_vector(const std::string& path, uint32_t rows) {
    std::FILE* f = std::fopen(path.c_str(), "r");
    if (!f) throw std::runtime_error("Failed to open initial vector");
    std::vector<double> v(rows, 0.0);
    for (uint32_t i = 0; i < rows; ++i) {
        if (std::fscanf(f, "%lg\n", &v[i]) != 1) {
            std::fclose(f);
            throw std::runtime_error("Failed to open initial vector");   // the reference's message for a short file too
        }
    }
    std::fclose(f);
    return v;
}

void fold_diagonal(Matrix& m, uint32_t n, double regularization) {
    std::vector<double> diag(n, 0.0);
    Matrix out;
    for (size_t e = 0; e < m.row.size(); ++e) {
        if (m.row[e] == m.col[e]) {
            diag[m.row[e]] = (double)m.val[e];
            continue;
        }
        out.row.push_back(m.row[e]);
        out.col.push_back(m.col[e]);
        out.val.push_back(m.val[e]);
    }
    for (uint32_t i = 0; i < n; ++i) {
        const double d = diag[i] + regularization;
        if (d == 0.0) continue;
        out.row.push_back(i);
        out.col.push_back(i);
        out.val.push_back((float)d);
    }
    m = std::move(out);
}

void write_singular_values(const std::string& path, const double* values, size_t n) {
    std::FILE* f = std::fopen(path.c_str(), "w");
    if (!f) throw std::runtime_error("Failed to open file: " + path + " for writing. ");
    std::fprintf(f, "%c%s\n", '%', "%GraphLab SVD Solver library. This file contains the singular values.");
    for (size_t j = 0; j < n; ++j) std::fprintf(f, "%10.13g\n", values[j]);
    std::fclose(f);
}

void write_vector(const std::string& prefix, int nshards, bool use_ids, uint32_t first_id, const double* values,
                  uint32_t n) {
    if (use_ids) {
        cfio::IdMap ids;
        std::vector<uint32_t> all(n);
        for (uint32_t i = 0; i < n; ++i) all[i] = first_id + i;
        ids.build(all);
        cfmf::write_vertex_values(ids, prefix, nshards, std::vector<double>(values, values + n), 1, " ", false);
        return;
    }
    cfio::ShardWriter w(".", prefix, nshards);
    for (uint32_t i = 0; i < n; ++i) {
        std::string& out = w.shard(first_id + i);
        cfmf::append_lex(out, values[i]);
        out += '\n';
    }
    w.flush();
}

}  // namespace cfsvdio

// ---- C wrappers for the tests (libcf_host.so) ------------------------------------------------

// Entries of the directory into row / col / val (capacity cap; 0-based).  Returns the entry
// count (call with cap = 0 for the size), or -1 on a fatal input (message in err, if given).
extern "C" int64_t cfh_svd_load(const char* dir, const char* vecfile, uint32_t rows, uint32_t cols, uint32_t* row,
                                uint32_t* col, float* val, int64_t cap, char* err, int err_cap) {
    try {
        const cfsvdio::Matrix m = cfsvdio::load_matrix(dir, vecfile ? vecfile : "", rows, cols);
        const int64_t n = (int64_t)m.row.size();
        if (n <= cap) {
            std::copy(m.row.begin(), m.row.end(), row);
            std::copy(m.col.begin(), m.col.end(), col);
            std::copy(m.val.begin(), m.val.end(), val);
        }
        return n;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) std::snprintf(err, (size_t)err_cap, "%s", e.what());
        return -1;
    }
}

extern "C" int cfh_svd_load_vector(const char* path, uint32_t rows, double* out) {
    try {
        const std::vector<double> v = cfsvdio::load_initial_vector(path, rows);
        std::copy(v.begin(), v.end(), out);
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

extern "C" int cfh_svd_write_values(const char* path, const double* values, uint64_t n) {
    try {
        cfsvdio::write_singular_values(path, values, (size_t)n);
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}

extern "C" int cfh_svd_write_vector(const char* prefix, int nshards, int use_ids, uint32_t first_id, const double* values,
                                    uint32_t n) {
    try {
        cfsvdio::write_vector(prefix, nshards, use_ids != 0, first_id, values, n);
        return 0;
    } catch (const std::exception&) {
        return -1;
    }
}
