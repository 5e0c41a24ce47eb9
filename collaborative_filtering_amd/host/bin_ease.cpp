// ease -- EASE (Steck, WWW 2019), the closed-form linear item-item model, fitted on the TRAIN edges of
// a movielens/ directory and used at once: lists for every user, or the ranking metrics of the
// VALIDATE edges.  No reference counterpart.  The weights are not saved: they are n_items^2 doubles
// and a refit takes seconds.
//   ease --matrix DIR --lambda L [--binary] [--recommend R --topn N [--users FILE] [--nshards 4]]
//        [--rankeval [--cutoff N] [--weighted] [--output R]]
//   --matrix DIR     the loader of the factor binaries (cf_mf_cli.hpp); a TRAIN pair listed twice keeps
//                    its last value; users and items are those of every role of DIR
//   --lambda L       the ridge term, > 0
//   --binary         every TRAIN edge counts as 1, in the fit and in the profiles
//   --recommend R    R_<i>_of_<nshards>: the --topn best items per user, TRAIN and VALIDATE edges
//                    excluded, in the format of recommend (cf_rank_cli.hpp)
//   --rankeval       TRAIN edges excluded, VALIDATE edges held out; the two metric lines of rankeval at
//                    --cutoff (default 10), --weighted and --output as there
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "cf_mf_cli.hpp"
#include "cf_rank_cli.hpp"

int main(int argc, char** argv) {
    const std::string matrix = cfcli::opt(argc, argv, "matrix", "");
    const std::string lambda_s = cfcli::opt(argc, argv, "lambda", "");
    const std::string recommend = cfcli::opt(argc, argv, "recommend", "");
    const std::string topn = cfcli::opt(argc, argv, "topn", "");
    const std::string users_file = cfcli::opt(argc, argv, "users", "");
    const std::string output = cfcli::opt(argc, argv, "output", "");
    const std::string cutoff_s = cfcli::opt(argc, argv, "cutoff", "10");
    const int nshards = std::stoi(cfcli::opt(argc, argv, "nshards", "4"));
    bool binary = false, rankeval = false, weighted = false;
    for (int i = 1; i < argc; ++i) {
        binary = binary || std::strcmp(argv[i], "--binary") == 0;
        rankeval = rankeval || std::strcmp(argv[i], "--rankeval") == 0;
        weighted = weighted || std::strcmp(argv[i], "--weighted") == 0;
    }
    const char* usage =
        "usage: ease --matrix DIR --lambda L [--binary] [--recommend R --topn N [--users FILE] [--nshards 4]]\n"
        "            [--rankeval [--cutoff N] [--weighted] [--output R]]";
    if (matrix.empty() || lambda_s.empty()) cfcli::die(usage);
    if (!recommend.empty() && topn.empty()) cfcli::die(usage);
    const double lambda = std::stod(lambda_s);
    if (!std::isfinite(lambda) || !(lambda > 0.0)) cfcli::die("--lambda must be finite and above 0");
    const uint32_t N = recommend.empty() ? 1 : (uint32_t)std::stoul(topn);
    const uint32_t cutoff = (uint32_t)std::stoul(cutoff_s);
    if (N == 0 || N > CF_TOPN_MAX_N) cfcli::die("--topn must be between 1 and " + std::to_string(CF_TOPN_MAX_N));
    if (cutoff == 0 || cutoff > CF_TOPN_MAX_N) cfcli::die("--cutoff must be between 1 and " + std::to_string(CF_TOPN_MAX_N));
    if (nshards < 1) cfcli::die("--nshards must be at least 1");

    const double inf = std::numeric_limits<double>::infinity();
    const cfmf::Data d = cfmf::load(matrix, -inf, inf);
    const uint32_t nu = d.nu, nm = d.nm;

    // the TRAIN edges by user, then item; of a pair listed twice the last line stays
    std::vector<std::tuple<uint32_t, uint32_t, float>> train;
    for (size_t e = 0; e < d.eu[cfio::kTrain].size(); ++e)
        train.emplace_back(d.eu[cfio::kTrain][e], d.em[cfio::kTrain][e], d.eo[cfio::kTrain][e]);
    std::stable_sort(train.begin(), train.end(), [](const auto& a, const auto& b) {
        return std::get<0>(a) != std::get<0>(b) ? std::get<0>(a) < std::get<0>(b) : std::get<1>(a) < std::get<1>(b);
    });
    std::vector<uint32_t> tu, tm;
    std::vector<float> to;
    for (size_t e = 0; e < train.size(); ++e) {
        if (e + 1 < train.size() && std::get<0>(train[e]) == std::get<0>(train[e + 1]) &&
            std::get<1>(train[e]) == std::get<1>(train[e + 1]))
            continue;
        tu.push_back(std::get<0>(train[e]));
        tm.push_back(std::get<1>(train[e]));
        to.push_back(std::get<2>(train[e]));
    }
    cfmf::Csr prof = cfmf::build_csr(nu, tu, tm, to);
    const uint64_t nnz = prof.nbr.size();
    if (prof.nbr.empty()) {   // valid pointers for an empty list
        prof.nbr.push_back(0);
        prof.obs.push_back(0.0f);
    }

    cf_ctx* ctx = cfcli::open_device();
    cfcli::check(ctx, cf_ease_fit(ctx, nu, nm, prof.off.data(), prof.nbr.data(), prof.obs.data(), binary ? 1 : 0, lambda),
                 "cf_ease_fit");
    float ms[3] = {0.0f, 0.0f, 0.0f};
    cfcli::check(ctx, cf_ease_timing(ctx, ms), "cf_ease_timing");
    std::printf("EASE fit: users: %u items: %u nnz: %llu  gram: %.3f ms  invert: %.3f ms  normalise: %.3f ms\n", nu, nm,
                (unsigned long long)nnz, ms[0], ms[1], ms[2]);

    if (!recommend.empty()) {
        // exclusions: the TRAIN and VALIDATE edges
        std::vector<uint32_t> eu(d.eu[cfio::kTrain]), em(d.em[cfio::kTrain]);
        eu.insert(eu.end(), d.eu[cfio::kValidate].begin(), d.eu[cfio::kValidate].end());
        em.insert(em.end(), d.em[cfio::kValidate].begin(), d.em[cfio::kValidate].end());
        cfmf::Csr excl = cfmf::build_csr(nu, eu, em, std::vector<float>(eu.size(), 0.0f));
        if (excl.nbr.empty()) excl.nbr.push_back(0);
        cfrank::Lists l = cfrank::make_lists(users_file, d.uids, matrix, nu, N);
        cf_topn_stats st{};
        cfcli::check(ctx,
                     cf_ease_topn(ctx, nu, prof.off.data(), prof.nbr.data(), prof.obs.data(), binary ? 1 : 0,
                                  excl.off.data(), excl.nbr.data(), l.n_sel(), l.sel_ptr(), N, l.items.data(),
                                  l.scores.data(), l.count.data(), &st),
                     "cf_ease_topn");
        cfrank::print_topn_stats(st);
        cfrank::write_lists(recommend, nshards, d.uids, d.mids, l);
    }

    if (rankeval) {
        cfmf::Csr excl = cfmf::build_csr(nu, d.eu[cfio::kTrain], d.em[cfio::kTrain],
                                         std::vector<float>(d.eu[cfio::kTrain].size(), 0.0f));
        if (excl.nbr.empty()) excl.nbr.push_back(0);
        std::vector<std::tuple<uint32_t, uint32_t, float>> held;
        for (size_t e = 0; e < d.eu[cfio::kValidate].size(); ++e)
            held.emplace_back(d.eu[cfio::kValidate][e], d.em[cfio::kValidate][e], d.eo[cfio::kValidate][e]);
        const cfrank::Held h = cfrank::build_held(std::move(held), nu, d.uids, d.mids, matrix);
        std::vector<uint32_t> rank(h.item.size(), 0);
        std::vector<cf_rank_user> users((size_t)nu + 1);
        cf_rank_summary s{};
        cfcli::check(ctx,
                     cf_ease_rank_eval(ctx, nu, prof.off.data(), prof.nbr.data(), prof.obs.data(), binary ? 1 : 0,
                                       excl.off.data(), excl.nbr.data(), h.off.data(), h.item.data(),
                                       weighted ? h.w.data() : nullptr, cutoff, rank.data(), users.data(), &s),
                     "cf_ease_rank_eval");
        cfrank::print_rank_summary(s, h.n);
        if (!output.empty()) cfrank::write_ranks(output, nshards, d.uids, d.mids, h, rank, users);
    }
    cf_destroy(ctx);
    return 0;
}
