// svdpp -- drop-in for svdpp.cpp: SVD++ (bias-SGD plus the implicit-feedback item factors) on the
// GPU.  Everything is cfmf::svdpp_main (cf_mf_cli.hpp).
#include "cf_mf_cli.hpp"

int main(int argc, char** argv) { return cfmf::svdpp_main(argc, argv); }
