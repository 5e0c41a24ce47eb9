// cf_svd_io.hpp -- the file contract of svd.cpp (bin/svd's loader and writers), apart from the
// binary so that tests reach it through libcf_host.so (the cfh_svd_* wrappers in cf_svd_io.cpp).
//   svd.cpp:251-284  loader: every file of the directory except the initial-vector file and names
//                    ending in "singular_values" or "_v0"; lines "row col value", 1-based ids,
//                    the value parsed as a float; row > rows is fatal (here col > cols too, where
//                    the reference would index past its vertices)
//   svd.cpp:650-666  initial vector: `rows` values, one per line
//   svd.cpp:512-525  singular_values: "%c%s\n" of '%' and a comment that starts with '%' itself
//                    (so the header shows "%%"), then "%10.13g" per value
//   svd.cpp:173-218  U.<i> / V.<i>: one value per vertex, 17 significant digits, with --id
//                    preceded by "id ": rows 1-based, columns by their raw vertex id (rows + c, or
//                    c for a square matrix, 0-based)
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace cfsvdio {

struct Matrix {   // 0-based entries in file order
    std::vector<uint32_t> row, col;
    std::vector<float> val;
};

// Throws std::runtime_error with the message to die with.
Matrix load_matrix(const std::string& dir, const std::string& vecfile, uint32_t rows, uint32_t cols);
std::vector<double> load_initial_vector(const std::string& path, uint32_t rows);

// A square matrix keeps its diagonal apart in the reference (A_ii, the last line of a vertex wins,
// svd.cpp:276-280) and adds --regularization to it in every product (math.hpp:137-138): entry
// (i, i) becomes (float)(A_ii + regularization) wherever that is not 0.
void fold_diagonal(Matrix& m, uint32_t n, double regularization);

void write_singular_values(const std::string& path, const double* values, size_t n);

// One value per vertex into the shards of `prefix` (cfio::ShardWriter: the shard of vertex id
// first_id + i); with use_ids through cfmf::write_vertex_values ("id value").
void write_vector(const std::string& prefix, int nshards, bool use_ids, uint32_t first_id, const double* values,
                  uint32_t n);

}  // namespace cfsvdio
