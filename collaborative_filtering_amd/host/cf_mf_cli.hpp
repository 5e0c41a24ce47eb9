// cf_mf_cli.hpp -- what the matrix-factorization drop-ins (bin_als, bin_sgd, bin_biassgd,
// bin_svdpp) share: the three-role movielens/ loader with the fatal range check, the TRAIN CSRs,
// the reproducible initial factors, the writers of P, P.U and P.V, sgd_main(), all of bin_sgd and
// bin_biassgd but the switch between them, and svdpp_main(), all of bin_svdpp.
// Initial factors: the reference draws them with Eigen's setRandom() (als.cpp:103, sgd.cpp:104),
// i.e. the C library's rand() stream in vertex-construction order, which is not reproducible.
// Here factor d of the vertex with compact index i on side s (0 users, 1 items; compact = rank
// of its id among the side's sorted ids) is 2 u - 1 with
//   u = (splitmix64(splitmix64(seed + 0x9E3779B97F4A7C15 * (s + 1)) ^ (64 i + d)) >> 11) * 2^-53,
// uniform in [-1, 1): runs differ from the reference's by their starting point only.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "cf_cli.hpp"

namespace cfmf {

inline uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

inline void init_factors(std::vector<double>& F, uint32_t n, uint32_t D, uint64_t seed, int side) {
    const uint64_t key = splitmix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(side + 1));
    F.resize((size_t)n * D);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t d = 0; d < D; ++d)
            F[(size_t)i * D + d] = 2.0 * ((double)(splitmix64(key ^ (64ull * i + d)) >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}

// The first argument that is neither an option nor an option's value (add_positional("matrix")).
inline std::string positional(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        if (std::strncmp(argv[i], "--", 2) == 0) {
            if (!std::strchr(argv[i], '=')) ++i;
            continue;
        }
        return argv[i];
    }
    return "";
}

// --matrix DIR or the positional argument; prints the reference's parse error and exits without one.
inline std::string matrix_dir(int argc, char** argv) {
    std::string dir = cfcli::opt(argc, argv, "matrix", "");
    if (dir.empty()) dir = positional(argc, argv);
    if (dir.empty()) {
        std::printf("Error in parsing command line arguments.\n");
        std::exit(1);
    }
    return dir;
}

// boost::lexical_cast<std::string>(double): 17 significant digits
inline void append_lex(std::string& out, double v) {
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
inline Csr build_csr(uint32_t n_rows, const std::vector<uint32_t>& row, const std::vector<uint32_t>& col,
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

// The ratings of a movielens/ directory by role, over compact ids.
struct Data {
    cfio::IdMap uids, mids;   // every role makes vertices
    uint32_t nu = 0, nm = 0;
    std::vector<uint32_t> eu[3], em[3];
    std::vector<float> eo[3];
    std::vector<double> out_degree;   // per user, num_out_edges: every role
    Csr by_user, by_item;             // TRAIN only
};

// Prints "Loading graph." and the edge-count line; a TRAIN or VALIDATE rating outside
// [minval, maxval] is fatal (als.cpp:407-410, sgd.cpp:491-494, biassgd.cpp:537-540).
inline Data load(const std::string& dir, double minval, double maxval) {
    std::printf("Loading graph.\n");
    const std::vector<cfio::RoleRating> rs = cfio::load_movielens_roles(dir);
    std::vector<uint32_t> all_u, all_m;
    for (const auto& r : rs) {
        if (r.role != cfio::kPredict && ((double)r.obs < minval || (double)r.obs > maxval)) {
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
    Data d;
    d.uids.build(all_u);
    d.mids.build(all_m);
    d.nu = d.uids.size();
    d.nm = d.mids.size();
    d.out_degree.assign(d.nu, 0.0);
    for (const auto& r : rs) {
        const uint32_t u = d.uids.at[r.user], m = d.mids.at[r.item];
        d.eu[r.role].push_back(u);
        d.em[r.role].push_back(m);
        d.eo[r.role].push_back(r.obs);
        d.out_degree[u] += 1.0;
    }
    std::printf("Training edges: %zu validation edges: %zu\n", d.eu[cfio::kTrain].size(), d.eu[cfio::kValidate].size());
    d.by_user = build_csr(d.nu, d.eu[cfio::kTrain], d.em[cfio::kTrain], d.eo[cfio::kTrain]);
    d.by_item = build_csr(d.nm, d.em[cfio::kTrain], d.eu[cfio::kTrain], d.eo[cfio::kTrain]);
    return d;
}

// "Training RMSE: a[\tValidation RMSE: b]" from the two sums of squares (als.cpp:474-483).
inline std::string rmse_line(const Data& d, const double sq[2]) {
    std::string line = "Training RMSE: ";
    cfio::append_g(line, d.eu[0].empty() ? 0.0 : std::sqrt(sq[0] / (double)d.eu[0].size()));   // no TRAIN edge: 0, not 0/0
    if (!d.eu[1].empty()) {
        line += "\tValidation RMSE: ";
        cfio::append_g(line, std::sqrt(sq[1] / (double)d.eu[1].size()));
    }
    return line;
}

// P: "user\titem\tprediction" per PREDICT edge (als.cpp:504-506).
inline void write_predictions(const Data& d, const std::string& prefix, int nshards, const std::vector<double>& pred) {
    cfio::ShardWriter pw(".", prefix, nshards);
    for (size_t e = 0; e < pred.size(); ++e) {
        const uint32_t uid = d.uids.ids[d.eu[cfio::kPredict][e]];
        std::string& out = pw.shard(uid);
        cfio::append_u(out, uid);
        out += '\t';
        cfio::append_u(out, d.mids.ids[d.em[cfio::kPredict][e]]);
        out += '\t';
        cfio::append_g(out, pred[e]);
        out += '\n';
    }
    pw.flush();
}

// P.U / P.V: "id<sep>f0 f1 .. " per vertex, `width` values each, 17 significant digits.
inline void write_vertex_values(const cfio::IdMap& ids, const std::string& prefix, int nshards, const std::vector<double>& F,
                                uint32_t width, const char* sep, bool trailing_space) {
    cfio::ShardWriter w(".", prefix, nshards);
    for (uint32_t i = 0; i < ids.size(); ++i) {
        std::string& out = w.shard(ids.ids[i]);
        cfio::append_u(out, ids.ids[i]);
        out += sep;
        for (uint32_t d = 0; d < width; ++d) {
            append_lex(out, F[(size_t)i * width + d]);
            if (trailing_space) out += ' ';
        }
        out += '\n';
    }
    w.flush();
}

// "%8g  %8g[   %8g]": the reference's per-iteration line (setw(8) of time, training RMSE and
// validation RMSE, sgd.cpp:379-385).
inline void print_iteration(double seconds, double train_rmse, bool have_val, double val_rmse) {
    std::string line;
    char buf[40];
    std::snprintf(buf, sizeof(buf), "%8g  %8g", seconds, train_rmse);
    line += buf;
    if (have_val) {
        std::snprintf(buf, sizeof(buf), "   %8g", val_rmse);
        line += buf;
    }
    std::printf("%s\n", line.c_str());
}

// sgd (bias = false) and biassgd (bias = true): drop-ins for sgd.cpp / biassgd.cpp.
//   sgd.cpp:474-503 / biassgd.cpp:520-549   loader (as als.cpp's)
//   sgd.cpp:243-339 / biassgd.cpp:249-347   vertex program on the synchronous engine (cf_sgd_fit)
//   sgd.cpp:344-401 / biassgd.cpp:350-409   error aggregate, one line per user superstep (the trace)
//   sgd.cpp:404-467 / biassgd.cpp:412-513   --predictions P: P, P.U, P.V (bias: P.bias.U, P.bias.V)
//   sgd.cpp:540-565 / biassgd.cpp:599-624   options
// Deviations: --max_iter or --max_supersteps is mandatory (the reference never stops without
// one); --interval must be 0 (any other value makes the reference's step decay depend on wall
// clock time); the initial factors are this header's; the time column is the fit's wall time
// spread evenly over its user supersteps (the fit is one call).
inline int sgd_main(int argc, char** argv, bool bias) {
    const std::string dir = matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const std::string max_iter = cfcli::opt(argc, argv, "max_iter", "");
    cf_sgd_params par{};
    par.max_updates = max_iter.empty() ? std::numeric_limits<uint64_t>::max() : std::stoull(max_iter);
    par.lambda = std::stod(cfcli::opt(argc, argv, "lambda", "0.001"));
    par.gamma = std::stod(cfcli::opt(argc, argv, "gamma", "0.001"));
    par.step_dec = std::stod(cfcli::opt(argc, argv, "step_dec", "0.9"));
    par.tol = std::stod(cfcli::opt(argc, argv, "tol", "1e-3"));
    par.maxval = std::stod(cfcli::opt(argc, argv, "maxval", "1e+100"));
    par.minval = std::stod(cfcli::opt(argc, argv, "minval", "-1e+100"));
    par.max_supersteps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_supersteps", "0"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    // --engine is accepted and ignored (one engine)
    if (std::stoul(cfcli::opt(argc, argv, "interval", "0")) != 0)
        cfcli::die("--interval other than 0 is not supported (it ties the step decay to wall-clock time)");
    if (std::stoi(cfcli::opt(argc, argv, "implicitratingtype", "0")) != 0)
        cfcli::die("--implicitratingtype other than 0 (implicit.hpp's added edges) is not supported");
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));
    if (max_iter.empty() && par.max_supersteps == 0)
        cfcli::die("--max_iter or --max_supersteps is required (without a cap the run never ends)");

    const Data data = load(dir, par.minval, par.maxval);
    const uint32_t nu = data.nu, nm = data.nm;
    const auto& eu = data.eu;
    const auto& em = data.em;
    const auto& eo = data.eo;
    if (bias) {   // biassgd.cpp:684-687
        double sum = 0.0;
        for (float o : eo[cfio::kTrain]) sum += (double)o;
        par.global_mean = sum / (double)eo[cfio::kTrain].size();
        std::string line = "Global mean is: ";
        cfio::append_g(line, par.global_mean);
        std::printf("%s\n", line.c_str());
    }
    std::vector<double> U, V, bu, bi;
    init_factors(U, nu, D, seed, 0);
    init_factors(V, nm, D, seed, 1);
    if (bias) {
        bu.assign(nu, 0.0);
        bi.assign(nm, 0.0);
    }
    std::vector<uint32_t> nup_u(nu, 0), nup_m(nm, 0);
    // one trace row per user superstep, bounded by whichever cap is set
    uint64_t rows = par.max_supersteps ? (par.max_supersteps + 1) / 2 : std::numeric_limits<uint64_t>::max();
    if (!max_iter.empty()) rows = std::min<uint64_t>(rows, par.max_updates + 1);
    if (rows > (1u << 24)) cfcli::die("more than 2^24 user supersteps asked for");
    std::vector<double> trace(2 * (size_t)rows, 0.0);

    cf_ctx* ctx = cfcli::open_device();
    std::printf(bias ? "Running Bias-SGD\n" : "Running SGD\n");
    std::printf("Time   Training    Validation\n       RMSE        RMSE \n");
    cf_sgd_stats st{};
    const auto t0 = std::chrono::steady_clock::now();
    // every user has an out-edge (it would not be a vertex otherwise): all are signalled (sgd.cpp:335-339)
    cfcli::check(ctx,
                 cf_sgd_fit(ctx, nu, nm, D, data.by_user.off.data(), data.by_user.nbr.data(), data.by_user.obs.data(),
                            data.by_item.off.data(), data.by_item.nbr.data(), data.by_item.obs.data(), &par, U.data(),
                            V.data(), bias ? bu.data() : nullptr, bias ? bi.data() : nullptr, nup_u.data(), nup_m.data(),
                            nullptr, eu[1].size(), eu[1].data(), em[1].data(), eo[1].data(), trace.data(), (uint32_t)rows,
                            &st),
                 "cf_sgd_fit");
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const uint32_t done = (st.supersteps + 1) / 2;
    for (uint32_t t = 0; t < done && t < rows; ++t)
        print_iteration(wall * (t + 1) / done, eu[0].empty() ? 0.0 : std::sqrt(trace[2 * t] / (double)eu[0].size()),
                        !eu[1].empty(), eu[1].empty() ? 0.0 : std::sqrt(trace[2 * t + 1] / (double)eu[1].size()));
    if (st.n_nan)   // sgd.cpp:261-262
        cfcli::die("Got into numeric errors.. try to tune step size and regularization using --lambda and --gamma flags");
    std::printf("----------------------------------------------------------\n");
    std::printf("Supersteps: %u  reduction kernels: %.3f ms  apply kernels: %.3f ms\n", st.supersteps, st.reduce_ms,
                st.apply_ms);
    std::printf("Updates executed: %llu\n", (unsigned long long)st.updates);
    std::printf("Messages sent: %llu\n", (unsigned long long)st.messages);
    std::printf("Final error: \n");
    double sq[2] = {0.0, 0.0};
    for (int role = 0; role < 2; ++role)
        cfcli::check(ctx,
                     cf_sgd_error(ctx, eu[role].size(), eu[role].data(), em[role].data(), eo[role].data(), nu, nm, D,
                                  U.data(), V.data(), bias ? bu.data() : nullptr, bias ? bi.data() : nullptr,
                                  par.global_mean, par.minval, par.maxval, &sq[role]),
                     "cf_sgd_error");
    std::printf("%s\n", rmse_line(data, sq).c_str());

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        // sgd.cpp:418-419 saves the dot product as it is, biassgd.cpp:423-428 clamps
        cfcli::check(ctx,
                     cf_sgd_predict(ctx, np, eu[cfio::kPredict].data(), em[cfio::kPredict].data(), nu, nm, D, U.data(),
                                    V.data(), bias ? bu.data() : nullptr, bias ? bi.data() : nullptr, par.global_mean,
                                    bias ? 1 : 0, par.minval, par.maxval, pred.data()),
                     "cf_sgd_predict");
        write_predictions(data, predictions, nshards, pred);
        // sgd.cpp:435,456 write "id) ", biassgd.cpp:444,465 "id "
        write_vertex_values(data.uids, predictions + ".U", nshards, U, D, bias ? " " : ") ", true);
        write_vertex_values(data.mids, predictions + ".V", nshards, V, D, bias ? " " : ") ", true);
        if (bias) {   // biassgd.cpp:478-510: id then bias
            write_vertex_values(data.uids, predictions + ".bias.U", nshards, bu, 1, " ", false);
            write_vertex_values(data.mids, predictions + ".bias.V", nshards, bi, 1, " ", false);
        }
    }
    cf_destroy(ctx);
    return 0;
}

// svdpp: drop-in for svdpp.cpp.
//   svdpp.cpp:587-610   loader (as als.cpp's); the .validate and .predict edges are the implicit list
//   svdpp.cpp:268-397   vertex program on the synchronous engine (cf_svdpp_fit)
//   svdpp.cpp:412-476   error aggregate, one line per user superstep of either phase (the trace)
//   svdpp.cpp:479-578,790-807   --predictions P: P, P.U, P.V, P.bias.U, P.bias.V (the weights are not saved)
//   svdpp.cpp:664-697   options; --lambda, --gamma and --tol are parsed and never used there: accepted, ignored
// Deviations: those of sgd_main; the biases start at 0 (the reference never initialises them).
// Initial values: pvec is init_factors(seed, side) as for sgd; weight is the same draw with the
// side numbers 2 (users, W) and 3 (items, Y), so the four matrices are independent streams.
// --max_iter counts phase-1 and phase-2 updates alike: --max_iter 2k gives k gradient passes.
inline int svdpp_main(int argc, char** argv) {
    const std::string dir = matrix_dir(argc, argv);
    const uint32_t D = (uint32_t)std::stoul(cfcli::opt(argc, argv, "D", "20"));
    const std::string max_iter = cfcli::opt(argc, argv, "max_iter", "");
    cf_svdpp_params par{};
    par.max_updates = max_iter.empty() ? std::numeric_limits<uint64_t>::max() : std::stoull(max_iter);
    par.user_bias_step = std::stof(cfcli::opt(argc, argv, "user_bias_step", "1e-4"));
    par.user_bias_reg = std::stof(cfcli::opt(argc, argv, "user_bias_reg", "1e-4"));
    par.item_bias_step = std::stof(cfcli::opt(argc, argv, "item_bias_step", "1e-4"));
    par.item_bias_reg = std::stof(cfcli::opt(argc, argv, "item_bias_reg", "1e-4"));
    par.user_factor_step = std::stof(cfcli::opt(argc, argv, "user_factor_step", "1e-4"));
    par.user_factor_reg = std::stof(cfcli::opt(argc, argv, "user_factor_reg", "1e-4"));
    par.item_factor_step = std::stof(cfcli::opt(argc, argv, "item_factor_step", "1e-4"));
    par.item_factor_reg = std::stof(cfcli::opt(argc, argv, "item_factor_reg", "1e-4"));
    par.item_factor2_step = std::stof(cfcli::opt(argc, argv, "item_factor2_step", "1e-4"));
    par.item_factor2_reg = std::stof(cfcli::opt(argc, argv, "item_factor2_reg", "1e-4"));
    par.step_dec = std::stod(cfcli::opt(argc, argv, "step_dec", "0.9"));
    par.maxval = std::stod(cfcli::opt(argc, argv, "maxval", "1e+100"));
    par.minval = std::stod(cfcli::opt(argc, argv, "minval", "-1e+100"));
    par.max_supersteps = (uint32_t)std::stoul(cfcli::opt(argc, argv, "max_supersteps", "0"));
    const std::string predictions = cfcli::opt(argc, argv, "predictions", "");
    const uint64_t seed = std::stoull(cfcli::opt(argc, argv, "seed", "0"));
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    if (std::stoul(cfcli::opt(argc, argv, "interval", "0")) != 0)
        cfcli::die("--interval other than 0 is not supported (it ties the step decay to wall-clock time)");
    if (std::stoi(cfcli::opt(argc, argv, "implicitratingtype", "0")) != 0)
        cfcli::die("--implicitratingtype other than 0 (implicit.hpp's added edges) is not supported");
    if (D == 0 || D > CF_ALS_MAX_D) cfcli::die("--D must be between 1 and " + std::to_string(CF_ALS_MAX_D));
    if (max_iter.empty() && par.max_supersteps == 0)
        cfcli::die("--max_iter or --max_supersteps is required (without a cap the run never ends)");

    const Data data = load(dir, par.minval, par.maxval);
    const uint32_t nu = data.nu, nm = data.nm;
    const auto& eu = data.eu;
    const auto& em = data.em;
    const auto& eo = data.eo;
    {   // svdpp.cpp:758-761
        double sum = 0.0;
        for (float o : eo[cfio::kTrain]) sum += (double)o;
        par.global_mean = eo[cfio::kTrain].empty() ? 0.0 : sum / (double)eo[cfio::kTrain].size();
        std::string line = "Global mean is: ";
        cfio::append_g(line, par.global_mean);
        std::printf("%s\n", line.c_str());
    }
    // the implicit list: the VALIDATE edges, then the PREDICT edges, by user
    std::vector<uint32_t> iu(eu[1]), im(em[1]);
    iu.insert(iu.end(), eu[2].begin(), eu[2].end());
    im.insert(im.end(), em[2].begin(), em[2].end());
    const Csr imp = build_csr(nu, iu, im, std::vector<float>(iu.size(), 0.0f));
    std::vector<double> U, V, W, Y, bu(nu, 0.0), bi(nm, 0.0);
    init_factors(U, nu, D, seed, 0);
    init_factors(V, nm, D, seed, 1);
    init_factors(W, nu, D, seed, 2);
    init_factors(Y, nm, D, seed, 3);
    std::vector<uint32_t> nup_u(nu, 0), nup_m(nm, 0);
    uint64_t rows = par.max_supersteps ? (par.max_supersteps + 1) / 2 : std::numeric_limits<uint64_t>::max();
    if (!max_iter.empty()) rows = std::min<uint64_t>(rows, par.max_updates + 1);
    if (rows > (1u << 24)) cfcli::die("more than 2^24 user supersteps asked for");
    std::vector<double> trace(2 * (size_t)rows, 0.0);

    cf_ctx* ctx = cfcli::open_device();
    std::printf("Running SVD++\n");
    std::printf("Time   Training    Validation\n       RMSE        RMSE \n");
    cf_svdpp_stats st{};
    const auto t0 = std::chrono::steady_clock::now();
    cfcli::check(ctx,
                 cf_svdpp_fit(ctx, nu, nm, D, data.by_user.off.data(), data.by_user.nbr.data(), data.by_user.obs.data(),
                              data.by_item.off.data(), data.by_item.nbr.data(), data.by_item.obs.data(), imp.off.data(),
                              imp.nbr.data(), &par, U.data(), V.data(), W.data(), Y.data(), bu.data(), bi.data(),
                              nup_u.data(), nup_m.data(), nullptr, eu[1].size(), eu[1].data(), em[1].data(), eo[1].data(),
                              trace.data(), (uint32_t)rows, &st),
                 "cf_svdpp_fit");
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const uint32_t done = (st.supersteps + 1) / 2;
    for (uint32_t t = 0; t < done && t < rows; ++t)
        print_iteration(wall * (t + 1) / done, eu[0].empty() ? 0.0 : std::sqrt(trace[2 * t] / (double)eu[0].size()),
                        !eu[1].empty(), eu[1].empty() ? 0.0 : std::sqrt(trace[2 * t + 1] / (double)eu[1].size()));
    if (st.n_nan)   // svdpp.cpp:294-295
        cfcli::die("Got into numeric errors.. try to tune step size and regularization using command line flags");
    std::printf("----------------------------------------------------------\n");
    std::printf("Supersteps: %u  reduction kernels: %.3f ms  apply kernels: %.3f ms\n", st.supersteps, st.reduce_ms,
                st.apply_ms);
    std::printf("Updates executed: %llu\n", (unsigned long long)st.updates);
    std::printf("Messages sent: %llu\n", (unsigned long long)st.messages);
    std::printf("Final error: \n");
    double sq[2] = {0.0, 0.0};
    for (int role = 0; role < 2; ++role)   // extract_l2_error: without Y
        cfcli::check(ctx,
                     cf_sgd_error(ctx, eu[role].size(), eu[role].data(), em[role].data(), eo[role].data(), nu, nm, D,
                                  U.data(), V.data(), bu.data(), bi.data(), par.global_mean, par.minval, par.maxval,
                                  &sq[role]),
                     "cf_sgd_error");
    std::printf("%s\n", rmse_line(data, sq).c_str());

    if (!predictions.empty()) {
        std::printf("Saving predictions\n");
        const size_t np = eu[cfio::kPredict].size();
        std::vector<double> pred(np);
        cfcli::check(ctx,
                     cf_svdpp_predict(ctx, np, eu[cfio::kPredict].data(), em[cfio::kPredict].data(), nu, nm, D, U.data(),
                                      V.data(), Y.data(), bu.data(), bi.data(), par.global_mean, par.minval, par.maxval,
                                      pred.data()),
                     "cf_svdpp_predict");
        write_predictions(data, predictions, nshards, pred);
        write_vertex_values(data.uids, predictions + ".U", nshards, U, D, " ", true);   // svdpp.cpp:509-512: "id f0 f1 .. "
        write_vertex_values(data.mids, predictions + ".V", nshards, V, D, " ", true);
        write_vertex_values(data.uids, predictions + ".bias.U", nshards, bu, 1, " ", false);
        write_vertex_values(data.mids, predictions + ".bias.V", nshards, bi, 1, " ", false);
    }
    cf_destroy(ctx);
    return 0;
}

}  // namespace cfmf
