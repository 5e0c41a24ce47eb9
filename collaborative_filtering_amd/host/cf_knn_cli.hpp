// cf_knn_cli.hpp -- the --graph source of recommend and rankeval: the item graph of knn2 (the
// out_fin_ shards) uploaded as the context's graph, and the TRAIN edges of a movielens/ directory
// as the users' profiles for cf_knn_topn / cf_knn_rank_eval.
//   users    the users of DIR, ascending id
//   items    the ids of PREFIX* and of DIR together, ascending id
//   profile  the TRAIN edges of DIR by user, ascending item id within a user (the order the sums run)
//   weights  as parsed floats, like knn3 (bin_knn3.cpp); the threshold is the kernel's
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "cf_cli.hpp"
#include "cf_mf_cli.hpp"

namespace cfknn {

struct Options {
    std::string graph;   // empty: the factor source
    int score_mode = CF_KNN_SCORE_SUM;
    double w_min = 0.1;
};

// --graph PREFIX [--wmin W] [--score sum|mean]; exactly one of --factors / --graph, and with
// --graph a --matrix and neither --bias nor --mean.
inline Options options(int argc, char** argv, const std::string& factors, const std::string& matrix, const char* usage) {
    Options o;
    o.graph = cfcli::opt(argc, argv, "graph", "");
    if (o.graph.empty() == factors.empty()) cfcli::die(usage);
    if (o.graph.empty()) return o;
    if (matrix.empty()) cfcli::die("--graph needs --matrix DIR (the TRAIN edges are the profiles)");
    for (int i = 1; i < argc; ++i)
        if (std::strcmp(argv[i], "--bias") == 0 || std::strcmp(argv[i], "--mean") == 0 || std::strncmp(argv[i], "--mean=", 7) == 0)
            cfcli::die("--bias and --mean belong to --factors, not to --graph");
    const std::string score = cfcli::opt(argc, argv, "score", "sum");
    if (score == "mean") o.score_mode = CF_KNN_SCORE_MEAN;
    else if (score != "sum") cfcli::die("--score must be sum or mean");
    o.w_min = std::stod(cfcli::opt(argc, argv, "wmin", "0.1"));
    if (!(o.w_min >= 0.0) || o.w_min > 1e300) cfcli::die("--wmin must be finite and at least 0");
    return o;
}

struct Source {
    cfio::IdMap users, items;
    std::vector<cfio::RoleRating> roles;   // every line of DIR
    cfmf::Csr profile;
};

// Reads both inputs and uploads the graph into ctx.
inline Source load(cf_ctx* ctx, const std::string& graph, const std::string& matrix) {
    const size_t slash = graph.rfind('/');
    const std::string dir = slash == std::string::npos ? std::string(".") : graph.substr(0, slash + 1);
    const std::string base = slash == std::string::npos ? graph : graph.substr(slash + 1);
    std::vector<cfio::Edge> edges = cfio::load_edges(dir, base);
    if (edges.empty()) cfcli::die("no edge in " + graph + "*");
    Source s;
    s.roles = cfio::load_movielens_roles(matrix);
    std::vector<uint32_t> us, ms;
    for (const cfio::Edge& e : edges) {
        ms.push_back(e.a);
        ms.push_back(e.b);
    }
    for (const cfio::RoleRating& r : s.roles) {
        us.push_back(r.user);
        ms.push_back(r.item);
    }
    s.users.build(us);
    s.items.build(ms);
    for (cfio::Edge& e : edges) e.w = (double)(float)e.w;
    cfcli::upload_edges(ctx, s.items, edges);
    std::vector<std::tuple<uint32_t, uint32_t, float>> train;
    for (const cfio::RoleRating& r : s.roles)
        if (r.role == cfio::kTrain) train.emplace_back(s.users.at[r.user], s.items.at[r.item], r.obs);
    std::stable_sort(train.begin(), train.end(), [](const auto& a, const auto& b) {
        return std::get<0>(a) != std::get<0>(b) ? std::get<0>(a) < std::get<0>(b) : std::get<1>(a) < std::get<1>(b);
    });
    std::vector<uint32_t> tu, tm;
    std::vector<float> to;
    for (const auto& t : train) {
        tu.push_back(std::get<0>(t));
        tm.push_back(std::get<1>(t));
        to.push_back(std::get<2>(t));
    }
    s.profile = cfmf::build_csr(s.users.size(), tu, tm, to);
    if (s.profile.nbr.empty()) {   // valid pointers for an empty list
        s.profile.nbr.push_back(0);
        s.profile.obs.push_back(0.0f);
    }
    return s;
}

}  // namespace cfknn
