// als -- drop-in for als.cpp: ALS matrix factorization of movielens/ ratings on the GPU.
//   als.cpp:379-417  loader: role by file suffix (TRAIN, .validate, .predict), "user item [rating]",
//                    ratings outside [minval, maxval] are fatal for TRAIN and VALIDATE
//   als.cpp:290-371  vertex program on the synchronous engine (cf_als_fit)
//   als.cpp:424-483  error aggregate: RMSE per role of the clamped predictions (cf_als_error)
//   als.cpp:493-553  --predictions P: P (PREDICT edges), P.U (vertices with out-edges), P.V (the rest)
//   als.cpp:579-600  options
// Initial factors: the reference draws them with Eigen's setRandom() (als.cpp:103), i.e. the C
// library's rand() stream in vertex-construction order, which is not reproducible.  Here
// factor d of the vertex with compact index i on side s (0 users, 1 items; compact = rank of
// its id among the side's sorted ids) is 2 u - 1 with
//   u = (splitmix64(splitmix64(seed + 0x9E3779B97F4A7C15 * (s + 1)) ^ (64 i + d)) >> 11) * 2^-53,
// uniform in [-1, 1): runs differ from the reference's by their starting point only.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "cf_cli.hpp"

namespace {

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

void init_factors(std::vector<double>& F, uint32_t n, uint32_t D, uint64_t seed, int side) {
    const uint64_t key = splitmix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(side + 1));
    F.resize((size_t)n * D);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t d = 0; d < D; ++d)
            F[(size_t)i * D + d] = 2.0 * ((double)(splitmix64(key ^ (64ull * i + d)) >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}

// The first argument that is neither an option nor an option's value (add_positional("matrix")).
std::string positional(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        if (std::strncmp(argv[i], "--", 2) == 0) {
            if (!std::strchr(argv[i], '=')) ++i;
            continue;
        }
        return argv[i];
    }
    return "";
}

// boost::lexical_cast<std::string>(double): 17 significant digits
void append_lex(std::string& out, double v) {
    char buf[40];
    std::snprintf(buf, sizeof(buf), "%.17g", v);
    out += buf;
}

struct Csr {
    std::vector<uint64_t> off;
    std::vector<uint32_t> nbr;
    std::vector<float> obs;
};

// Stable CSR of the TRAIN edges by `row`.
Csr build_csr(uint32_t n_rows, const std::vector<uint32_t>& row, const std::vector<uint32_t>& col,
              const std::vector<float>& obs) {
    Csr c;
    c.off.assign((size_t)n_rows + 1, 0);
    for (uint32_t r : row) c.off[r + 1]++;
    for (uint32_t i = 0; i < n_rows; ++i) c.off[i + 1] += c.off[i];
    c.nbr.resize(row.size());
    c.obs.resize(row.size());
    std::vector<uint64_t> fill(c.off.begin(), c.off.end() - 1);
    for (size_t e = 0; e < row.size(); ++e) {
        const uint64_t p = fill[row[e]]++;
        c.nbr[p] = col[e];
        c.obs[p] = obs[e];
    }
    return c;
}

}  // namespace

int main(int argc, char** argv) {
    std::string dir = cfcli::opt(argc, argv, "matrix", "");
    if (dir.empty()) dir = positional(argc, argv);
    if (dir.empty()) {
        std::printf("Error in parsing command line arguments.\n");
        return 1;
    }
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const std::string max_iter = cfcli::opt(argc, argv, "max_iter", "");
    const uint64_t max_updates = max_iter.empty() ? std::numeric_limits<uint64_t>::max() : std::stoull(max_iter);
    const double lambda = std::stod(cfcli::opt(argc, argv, "lambda", "0.01"));
    const double tol = std::stod(cfcli::opt(argc, argv, "tol", "1e-3"));
    const double maxval = std::stod(cfcli::opt(argc, argv, "maxval", "1e+100"));
    const double minval = std::stod(cfcli::opt(argc, argv, "minval", "-1e+100"));
    const int regnormal = std::stoi(cfcli::opt(argc, argv, "regnormal", "1"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    const uint32_t max_supersteps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_supersteps", "0"));
    // --engine and --interval are accepted and ignored (one engine, one final report)
    if (std::stoi(cfcli::opt(argc, argv, "implicitratingtype", "0")) != 0)
        cfcli::die("--implicitratingtype other than 0 (implicit.hpp's added edges) is not supported");
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));

    std::printf("Loading graph.\n");
    const std::vector<cfio::RoleRating> rs = cfio::load_movielens_roles(dir);
    std::vector<uint32_t> all_u, all_m;
    for (const auto& r : rs) {
        if (r.role != cfio::kPredict && ((double)r.obs < minval || (double)r.obs > maxval)) {   // als.cpp:407-410
            std::string msg = "Rating values should be between ";
            cfio::append_g(msg, minval);
            msg += " and ";
            cfio::append_g(msg, maxval);
            msg += ". Got value: ";
            cfio::append_g(msg, r.obs);
            msg += " [ user: " + std::to_string(r.user) + " to item: " + std::to_string(r.item) + " ] ";
            cfcli::die(msg);
        }
        all_u.push_back(r.user);
        all_m.push_back(r.item);
    }
    cfio::IdMap uids, mids;   // every role makes vertices
    uids.build(all_u);
    mids.build(all_m);
    const uint32_t nu = uids.size(), nm = mids.size();
    std::vector<uint32_t> eu[3], em[3];
    std::vector<float> eo[3];
    std::vector<double> out_degree(nu, 0.0);   // num_out_edges: every role
    for (const auto& r : rs) {
        const uint32_t u = uids.at[r.user], m = mids.at[r.item];
        eu[r.role].push_back(u);
        em[r.role].push_back(m);
        eo[r.role].push_back(r.obs);
        out_degree[u] += 1.0;
    }
    std::printf("Training edges: %zu validation edges: %zu\n", eu[cfio::kTrain].size(), eu[cfio::kValidate].size());

    const Csr by_user = build_csr(nu, eu[cfio::kTrain], em[cfio::kTrain], eo[cfio::kTrain]);
    const Csr by_item = build_csr(nm, em[cfio::kTrain], eu[cfio::kTrain], eo[cfio::kTrain]);
    // regularisation (als.cpp:323-327): lambda, or lambda * num_out_edges -- 0 for every item
    std::vector<double> reg_u(nu, lambda), reg_m(nm, regnormal ? 0.0 : lambda);
    if (regnormal)
        for (uint32_t u = 0; u < nu; ++u) reg_u[u] = lambda * out_degree[u];
    std::vector<double> U, V;
    init_factors(U, nu, D, seed, 0);
    init_factors(V, nm, D, seed, 1);
    std::vector<uint32_t> nup_u(nu, 0), nup_m(nm, 0);
    std::vector<float> res_u(nu, 0.0f), res_m(nm, 0.0f);

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running ALS\n");
    cf_als_stats st{};
    // every user has an out-edge (it would not be a vertex otherwise): all are signalled (als.cpp:363-367)
    cfcli::check(ctx,
                 cf_als_fit(ctx, nu, nm, D, by_user.off.data(), by_user.nbr.data(), by_user.obs.data(), by_item.off.data(),
                            by_item.nbr.data(), by_item.obs.data(), reg_u.data(), reg_m.data(), tol, max_updates,
                            max_supersteps, U.data(), V.data(), nup_u.data(), nup_m.data(), res_u.data(), res_m.data(),
                            nullptr, &st),
                 "cf_als_fit");
    std::printf("----------------------------------------------------------\n");
    std::printf("Supersteps: %u  update kernels: %.3f ms  scatter kernels: %.3f ms\n", st.supersteps, st.update_ms,
                st.scatter_ms);
    std::printf("Updates executed: %llu\n", (unsigned long long)st.updates);
    if (st.n_not_pd)
        std::printf("warning: %llu pivots were not positive (systems outside the parity claim)\n",
                    (unsigned long long)st.n_not_pd);
    std::printf("Final error: \n");
    double sq[2] = {0.0, 0.0};
    for (int role = 0; role < 2; ++role)
        cfcli::check(ctx,
                     cf_als_error(ctx, eu[role].size(), eu[role].data(), em[role].data(), eo[role].data(), nu, nm, D,
                                  U.data(), V.data(), minval, maxval, &sq[role]),
                     "cf_als_error");
    std::string line = "Training RMSE: ";
    cfio::append_g(line, eu[0].empty() ? 0.0 : std::sqrt(sq[0] / (double)eu[0].size()));   // no TRAIN edge: 0, not 0/0
    if (!eu[1].empty()) {
        line += "\tValidation RMSE: ";
        cfio::append_g(line, std::sqrt(sq[1] / (double)eu[1].size()));
    }
    std::printf("%s\n", line.c_str());

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        cfcli::check(ctx,
                     cf_als_predict(ctx, np, eu[cfio::kPredict].data(), em[cfio::kPredict].data(), nu, nm, D, U.data(),
                                    V.data(), pred.data()),
                     "cf_als_predict");
        cfio::ShardWriter pw(".", predictions, nshards), uw(".", predictions + ".U", nshards),
            vw(".", predictions + ".V", nshards);
        for (size_t e = 0; e < np; ++e) {   // als.cpp:504-506
            const uint32_t uid = uids.ids[eu[cfio::kPredict][e]];
            std::string& out = pw.shard(uid);
            cfio::append_u(out, uid);
            out += '\t';
            cfio::append_u(out, mids.ids[em[cfio::kPredict][e]]);
            out += '\t';
            cfio::append_g(out, pred[e]);
            out += '\n';
        }
        for (int side = 0; side < 2; ++side) {   // als.cpp:521-525, 542-546
            const cfio::IdMap& ids = side ? mids : uids;
            const std::vector<double>& F = side ? V : U;
            cfio::ShardWriter& w = side ? vw : uw;
            for (uint32_t i = 0; i < ids.size(); ++i) {
                std::string& out = w.shard(ids.ids[i]);
                cfio::append_u(out, ids.ids[i]);
                out += side ? ") " : " ";
                for (uint32_t d = 0; d < D; ++d) {
                    append_lex(out, F[(size_t)i * D + d]);
                    out += ' ';
                }
                out += '\n';
            }
        }
        pw.flush();
        uw.flush();
        vw.flush();
    }
    cf_destroy(ctx);
    return 0;
}
