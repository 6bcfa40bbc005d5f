// hg_cli.cpp -- `hyper-gen` command line on top of libhypergen_hip.so.
//
// Mirrors the reference's CLI surface (src/utils.rs:42-162, src/main.rs:11-24): subcommands
// sketch / dist / search with the same flags and defaults, the same .sketch container and the
// same ANI TSV (src/utils.rs:260-308).  All arithmetic runs on the MI355X through the C ABI;
// `-D cpu|gpu` only selects which of the reference's two base-normalisation behaviours is
// reproduced (cpu: needletail, u/U -> T; gpu: src/cuda_kernel.cu, ACGTacgt only).
#include <fcntl.h>
#include <glob.h>
#include <sched.h>
#include <unistd.h>
#include <sys/stat.h>
#include <sys/uio.h>

#include <algorithm>
#include <atomic>
#include <bitset>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/hypergen.h"
#include "../../include/hypergen_aa.h"
#include "../../include/hypergen_frag.h"
#include "../../include/hypergen_hist.h"
#include "../../include/hypergen_rec.h"
#include "../../include/hypergen_tri.h"
#include "../../include/hypergen_tx.h"

namespace {

void logline(const char *lvl, const std::string &msg) {
  char ts[32];
  std::time_t t = std::time(nullptr);
  std::strftime(ts, sizeof ts, "%Y-%m-%d-%H:%M:%S", std::localtime(&t));  // src/utils.rs:17-29
  std::printf("%s [%s] - %s\n", ts, lvl, msg.c_str());
  std::fflush(stdout);
}

// RUST_LOG=debug (the reference logs through env_logger) adds per-stage timings
bool debug_log() {
  static const bool on = [] {
    const char *e = std::getenv("RUST_LOG");
    return e && std::strstr(e, "debug") != nullptr;
  }();
  return on;
}
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void debugf(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void debugf(const char *fmt, ...) {
  if (!debug_log()) return;
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  logline("DEBUG", buf);
}

[[noreturn]] void die(const std::string &msg) {
  std::fprintf(stderr, "error: %s\n", msg.c_str());
  std::fflush(nullptr);
  _exit(2);  // not exit(): reader threads, or a thread that is bringing the HIP runtime up, may still be running
}

enum class Linkage { single, greedy, setcover };
enum class SearchPath { automatic, hits, topk };  // automatic: topk whenever top_n <= HG_SEARCH_TOPK_MAX, else the hit list
enum : unsigned { SKETCH = 1, DIST = 2, SEARCH = 4, CLUSTER = 8, TRIANGLE = 16, ANY = 31 };  // subcommands, as bits of Option::modes

struct Cli {
  std::string mode, path = "1", path_r = "1", path_q = "1", out, method = "t1ha2", device = "cpu";
  unsigned mode_bit = 0;
  bool pack_naive = false;  // --pack_layout naive: the payload layout of reference hosts without AVX2 (src/hd.rs:158-166)
  unsigned shards = 0;      // --shards N (dist / search; testing aid): N shards dealt round the visible devices instead of one each
  unsigned threads = 16, ksize = 21, top_n = 1;
  bool canonical = true;
  unsigned long long seed = 123, scaled = 1500, hv_d = 4096;
  float quant_scale = 1.0f, ani_th = 85.0f;  // (cluster's default threshold is 95.0, the other subcommands' 85.0)
  bool protein = false;      // --alphabet dna|protein (sketch): protein = amino-acid k-mers of the *.faa files of -p (hypergen_aa.h)
  // (three switches have no field: --translate (sketch): amino-acid k-mers of the six reading frames of the nucleotide files
  // (hypergen_tx.h); --individual (sketch): one sketch per FASTA record of every file, the files split on the device
  // (hypergen_rec.h); --fragments (dist): fragment-wise ANI and aligned fraction per pair of genomes (hypergen_frag.h) --
  // given(c, "translate") and so on is all there is to know of them)
  unsigned long long min_length = 0;  // --min_length N (sketch --individual): leave out records with fewer than N sequence bytes
  unsigned long long fragment = 0, fragment_step = 0;  // --fragment W [--fragment_step S] (sketch): one sketch per window of W bases every S [W] bases of every file (hypergen_frag.h)
  float fragment_ani = 90.0f;        // --fragment_ani T (dist --fragments): a fragment counts as matched from this ANI of its best window on
  unsigned long long min_fragments = 1;  // --min_fragments N (dist --fragments): pairs with fewer matched fragments are not written
  std::string fragment_hits;         // --fragment_hits FILE (dist --fragments): one line per matched (reference genome, query fragment)
  unsigned min_count = 1;    // --min_count N (sketch): keep a sampled k-mer only if it occurs at least N times (hg_sketch_params.min_count)
  SearchPath search_path = SearchPath::automatic;  // --search_path auto|hits|topk (search; testing aid)
  int ani_metric = HG_ANI_MASH;  // --ani_metric mash|containment|max_containment (dist / search / cluster; hg_ctx_set_ani_metric)
  Linkage linkage = Linkage::single;  // --linkage single|greedy|setcover (cluster)
  bool order_size = false;     // --order file|size (cluster --linkage greedy)
  std::string tree_out;        // --tree <file> (cluster --linkage single): the single-linkage tree, one line per edge
  std::vector<float> levels;   // --levels L1,L2,... (cluster --linkage single): more thresholds, cut from the one tree
  bool hclust_average = false; // --hclust average, --agglomerate average (cluster): average linkage (UPGMA) on the dense matrix, a scheme of its own
  bool complete = false;       // --agglomerate complete (cluster): complete linkage on the dense matrix, likewise
  std::string stats_out;       // --stats <file> (cluster): medoid, cohesion and separation of every cluster at -a, one line each
  std::vector<uint32_t> columns;  // --columns LIST (dist): HG_PAIRS_* bits in the order listed, one further field per line each
  std::string pairs_file;         // --pairs FILE (dist): evaluate the listed name pairs instead of thresholding the matrix
  std::string newick_out;         // --newick <file> (dist on one file): the neighbour-joining tree of all its sketches
  std::string histogram_out;      // --histogram FILE (dist): the distribution of the ANI values of every pair of the comparison (hypergen_hist.h)
  uint32_t histogram_bin = 100;   // --histogram_bin B (dist --histogram): the width of a bin, an ANI, held in thousandths
  std::bitset<64> given;          // which options the command line carried, by row of `options`
};

// One option of the command line as it was typed, and the ways its value is read
struct Arg {
  std::string flag, val;  // "--thread=4", "-t4" or "-t", and "4"
  const char *name;       // the option's long name
  [[noreturn]] void bad(const std::string &tail = "") const { die("invalid value '" + val + "' for '--" + name + "'" + tail); }
  unsigned long long uint(unsigned long long max, unsigned long long min = 0) const {
    char *e = nullptr;
    const unsigned long long v = std::strtoull(val.c_str(), &e, 10);
    if (val.empty() || *e || v > max || v < min) die("invalid value '" + val + "' for '" + flag + "'");
    return v;
  }
  // the same, a bad value reported under the option's own name, "--thread", however the flag was typed
  unsigned long long named_uint(unsigned long long max, unsigned long long min = 0) const {
    return Arg{std::string("--") + name, val, name}.uint(max, min);
  }
  // the place of the value in a fixed list; the error names the list: " (a | b | c)"
  size_t choice(std::initializer_list<const char *> names, bool list_them = true) const {
    std::string list;
    for (const char *const *n = names.begin(); n != names.end(); ++n) {
      if (val == *n) return (size_t)(n - names.begin());
      list += std::string(n == names.begin() ? " (" : " | ") + *n;
    }
    bad(list_them ? list + ")" : "");
  }
  const std::string &file() const {
    if (val.empty()) bad(" (a file name)");
    return val;
  }
  std::vector<std::string> items() const {  // of a comma list, empty ones included
    std::vector<std::string> out;
    for (size_t b = 0, e; b <= val.size(); b = e + 1) out.push_back(val.substr(b, (e = std::min(val.find(',', b), val.size())) - b));
    return out;
  }
};

void take_levels(Cli &c, const Arg &a) {
  c.levels.clear();
  for (const std::string &item : a.items()) {
    char *end = nullptr;
    const float v = std::strtof(item.c_str(), &end);
    if (item.empty() || *end || !(v == v) || item.find_first_not_of("0123456789.+-eE") != std::string::npos)
      a.bad(" (1 to 8 ANI thresholds, comma-separated, ascending)");
    if (c.levels.size() == 8) a.bad(": at most 8 levels");
    if (!c.levels.empty() && !(v > c.levels.back())) a.bad(": the levels must be strictly ascending");
    c.levels.push_back(v);
  }
}
// --histogram_bin B: a decimal string into thousandths, exactly: digits, then at most three behind a point; 0.001 to 100
void take_histogram_bin(Cli &c, const Arg &a) {
  const char *const what = " (the width of a bin as an ANI: above 0, at most 100, at most three decimals)";
  const size_t point = std::min(a.val.find('.'), a.val.size());
  const std::string ip = a.val.substr(0, point), fp = point < a.val.size() ? a.val.substr(point + 1) : "";
  if (ip.size() + fp.size() == 0 || ip.size() > 6 || fp.size() > 3 || (ip + fp).find_first_not_of("0123456789") != std::string::npos) a.bad(what);
  uint64_t v = 0;
  for (const char ch : ip + fp + std::string(3 - fp.size(), '0')) v = v * 10 + (uint64_t)(ch - '0');
  if (v < 1 || v > HG_HIST_MILLI_MAX) a.bad(what);
  c.histogram_bin = (uint32_t)v;
}
void take_columns(Cli &c, const Arg &a) {
  static const std::pair<const char *, uint32_t> names[] = {{"mash", HG_PAIRS_MASH}, {"containment", HG_PAIRS_CONTAINMENT},
                                                            {"max_containment", HG_PAIRS_MAX_CONTAINMENT}, {"containment_ref", HG_PAIRS_CONTAINMENT_REF}};
  c.columns.clear();
  for (const std::string &item : a.items()) {
    uint32_t bit = 0;
    for (const auto &nm : names)
      if (item == nm.first) bit = nm.second;
    if (!bit) a.bad(" (a comma list out of mash, containment, containment_ref, max_containment)");
    if (std::find(c.columns.begin(), c.columns.end(), bit) != c.columns.end()) a.bad(": '" + item + "' is listed twice");
    c.columns.push_back(bit);
  }
}

// Every option: long name, short letter (0: none), how its value is taken (nullptr: a switch, it has none), the subcommands that
// accept it, why the others do not ("--name is not supported by <mode>: <why>") and why it does not go with --shards (nullptr:
// it does).  A subcommand that merely ignores an option accepts it, as the reference's one flat argument struct does
// (src/utils.rs:42-162).  The restricted rows stand in the order their faults are reported in.
struct Option {
  const char *name;
  char letter;
  void (*take)(Cli &, const Arg &);
  unsigned modes = ANY;
  const char *why = nullptr, *why_shards = nullptr;
};
const char *const ONE_GPU_CLUSTER = "cluster runs on the first visible GPU";
const char *const ONE_GPU_DIST = "dist with --columns or --pairs runs on the first visible GPU";
const Option options[] = {
    {"path", 'p', [](Cli &c, const Arg &a) { c.path = a.val; }},
    {"path_r", 'r', [](Cli &c, const Arg &a) { c.path_r = a.val; }},
    {"path_q", 'q', [](Cli &c, const Arg &a) { c.path_q = a.val; }},
    {"out", 'o', [](Cli &c, const Arg &a) { c.out = a.val; }},
    {"thread", 't', [](Cli &c, const Arg &a) { c.threads = (unsigned)a.uint(255); }},  // u8
    {"sketch_method", 'm', [](Cli &c, const Arg &a) { c.method = a.val; }},
    {"canonical", 'C', [](Cli &c, const Arg &a) { c.canonical = a.choice({"false", "true"}, false) == 1; }},
    {"ksize", 'k', [](Cli &c, const Arg &a) { c.ksize = (unsigned)a.uint(255); }},  // u8
    {"seed", 'S', [](Cli &c, const Arg &a) { c.seed = a.uint(~0ull); }},
    {"scaled", 's', [](Cli &c, const Arg &a) { c.scaled = a.uint(~0ull); }},
    {"hv_d", 'd', [](Cli &c, const Arg &a) { c.hv_d = a.uint(~0ull); }},
    {"quant_scale", 'Q', [](Cli &c, const Arg &a) { c.quant_scale = std::strtof(a.val.c_str(), nullptr); }},
    {"ani_th", 'a', [](Cli &c, const Arg &a) { c.ani_th = std::strtof(a.val.c_str(), nullptr); }},
    {"device", 'D', [](Cli &c, const Arg &a) { c.device = a.val; }},
    {"top_n", 'n', [](Cli &c, const Arg &a) { c.top_n = (unsigned)a.uint(1u << 20); }},  // (extension: the reference's search is a stub)
    // (extension) which of the reference's two payload layouts sketch writes
    {"pack_layout", 'L', [](Cli &c, const Arg &a) { c.pack_naive = a.val != "bitpacker8x" && a.choice({"avx2", "naive"}) == 1; }},
    {"ani_metric", 0, [](Cli &c, const Arg &a) {
       static const int metrics[] = {HG_ANI_MASH, HG_ANI_CONTAINMENT, HG_ANI_MAX_CONTAINMENT};
       c.ani_metric = metrics[a.choice({"mash", "containment", "max_containment"})];
     }},
    {"order", 0, [](Cli &c, const Arg &a) { c.order_size = a.choice({"file", "size"}) == 1; }},
    {"search_path", 0, [](Cli &c, const Arg &a) { c.search_path = SearchPath(a.choice({"auto", "hits", "topk"})); }, SEARCH,
     "it chooses how search selects its results"},
    {"linkage", 0, [](Cli &c, const Arg &a) { c.linkage = Linkage(a.choice({"single", "greedy", "setcover"})); }, CLUSTER,
     "it chooses how cluster forms its clusters"},
    {"tree", 0, [](Cli &c, const Arg &a) { c.tree_out = a.file(); }, CLUSTER, "it belongs to cluster --linkage single", ONE_GPU_CLUSTER},
    {"levels", 0, take_levels, CLUSTER, "it belongs to cluster --linkage single", ONE_GPU_CLUSTER},
    {"hclust", 0, [](Cli &c, const Arg &a) { c.hclust_average = a.choice({"average"}) == 0; }, CLUSTER,
     "it chooses the hierarchical clustering of cluster"},
    {"agglomerate", 0, [](Cli &c, const Arg &a) { c.complete = a.choice({"average", "complete"}) == 1, c.hclust_average = !c.complete; },
     CLUSTER, "it chooses the agglomerative clustering of cluster"},
    {"stats", 0, [](Cli &c, const Arg &a) { c.stats_out = a.file(); }, CLUSTER, "it describes the clusters of cluster", ONE_GPU_CLUSTER},
    {"columns", 0, take_columns, DIST, "it adds a pair's other metrics to the lines of dist", ONE_GPU_DIST},
    {"pairs", 0, [](Cli &c, const Arg &a) { c.pairs_file = a.file(); }, DIST, "it names the pairs dist evaluates", ONE_GPU_DIST},
    {"newick", 0, [](Cli &c, const Arg &a) { c.newick_out = a.file(); }, DIST, "it draws the tree of dist's comparison", ONE_GPU_DIST},
    {"min_count", 0, [](Cli &c, const Arg &a) { c.min_count = (unsigned)a.uint(0xFFFFFFFFull, 1); }, SKETCH,
     "the filter needs the k-mer counts, which a sketch no longer has"},
    // (testing aid: the several-GPU path on fewer GPUs)
    {"shards", 'G', [](Cli &c, const Arg &a) { c.shards = (unsigned)a.uint(64); }, SKETCH | DIST | SEARCH, "it runs on the first visible GPU"},
    // (sketch's other inputs and dist --fragments; their numbers are reported under the option's name: named_uint)
    {"alphabet", 0, [](Cli &c, const Arg &a) { c.protein = a.choice({"dna", "protein"}) == 1; }, SKETCH,
     "it names the alphabet of the sequences sketch reads"},
    {"translate", 0, nullptr, SKETCH, "it translates the nucleotide sequences sketch reads"},
    {"individual", 0, nullptr, SKETCH, "it splits the FASTA files sketch reads into their records"},
    {"min_length", 0, [](Cli &c, const Arg &a) { c.min_length = a.named_uint(~0ull); }, SKETCH, "it belongs to sketch --individual"},
    {"fragment", 0, [](Cli &c, const Arg &a) { c.fragment = a.named_uint(~0ull); }, SKETCH, "it cuts the sequences sketch reads into windows"},
    {"fragment_step", 0, [](Cli &c, const Arg &a) { c.fragment_step = a.named_uint(~0ull); }, SKETCH,
     "it cuts the sequences sketch reads into windows"},
    {"fragments", 0, nullptr, DIST, "it makes dist compare genomes fragment by fragment"},
    {"fragment_ani", 0, [](Cli &c, const Arg &a) {
       char *end = nullptr;
       c.fragment_ani = std::strtof(a.val.c_str(), &end);
       if (a.val.empty() || *end || !(c.fragment_ani >= 0.0f && c.fragment_ani <= 100.0f)) a.bad(" (an ANI, 0 to 100)");
     }, DIST, "it belongs to dist --fragments"},
    {"min_fragments", 0, [](Cli &c, const Arg &a) { c.min_fragments = a.named_uint(0xFFFFFFFFull, 1); }, DIST, "it belongs to dist --fragments"},
    {"fragment_hits", 0, [](Cli &c, const Arg &a) { c.fragment_hits = a.file(); }, DIST, "it belongs to dist --fragments"},
    // (dist --histogram, hypergen_hist.h: rows 41 and 42, the name on a line of its own; tests/test_hist_surface.py counts all rows)
    {"histogram",
     0, [](Cli &c, const Arg &a) { c.histogram_out = a.file(); }, DIST, "it counts the ANI values of dist's comparison",
     "dist with --histogram runs on the first visible GPU"},
    {"histogram_bin",
     0, take_histogram_bin, DIST, "it belongs to dist --histogram"},
};
const size_t N_OPTIONS = sizeof options / sizeof options[0];
static_assert(N_OPTIONS <= decltype(Cli::given)().size(), "Cli::given has a bit per row");

size_t option_row(const char *name) {
  for (size_t k = 0; k < N_OPTIONS; ++k)
    if (!std::strcmp(options[k].name, name)) return k;
  die(std::string("internal: no option --") + name);
}
bool given(const Cli &c, const char *name) { return c.given[option_row(name)]; }

// `hyper-gen --help`; `hyper-gen cluster --help` prints it too, with a paragraph on --hclust, one on --agglomerate and one on
// --stats behind it
void print_help() {
  std::printf("HyperGen: Fast and memory-efficient genome sketching in hyperdimensional space (MI355X build)\n\n"
              "  hyper-gen sketch -p {fna_path} -o {output_sketch_file}\n"
              "  hyper-gen dist -r {ref_sketch} -q {query_sketch} -o {output_ANI_results}\n"
              "  hyper-gen search -r {ref_sketch} -q {query_sketch} -o {top_hits_per_query} [-n top_n]\n"
              "  hyper-gen cluster -p {sketch_file} -o {output_clusters} [-a 95.0] [--linkage single|greedy|setcover]\n"
              "                    [--tree {output_tree}] [--levels L1,L2,...]\n\n"
              "options: -p --path, -r --path_r, -q --path_q, -o --out, -t --thread [16], -m --sketch_method,\n"
              "         -C --canonical [true], -k --ksize [21], -S --seed [123], -s --scaled [1500], -d --hv_d [4096],\n"
              "         -Q --quant_scale [1.0], -a --ani_th [85.0], -D --device [cpu]\n"
              "extensions: -n --top_n [1] (search), --pack_layout avx2|naive [avx2] (sketch: the payload layout of\n"
              "         reference hosts with / without AVX2; dist and search read both), --shards N (dist / search: N\n"
              "         shards dealt round the visible GPUs; default one per GPU), cluster (single-linkage clusters at\n"
              "         -a --ani_th [95.0] on the first visible GPU: one line per sketch, file, cluster id, file of the\n"
              "         cluster's first member), --ani_metric mash|containment|max_containment [mash] (dist / search /\n"
              "         cluster: containment = the share of the query's hashes found in the reference -- the identity of a\n"
              "         fragment, a partial MAG or a draft with a larger genome; max_containment = the same against the\n"
              "         smaller of the two; dist on one file with containment writes every ordered pair i != j; cluster\n"
              "         takes mash or max_containment), --min_count N [1] (sketch: keep a sampled k-mer only if it occurs\n"
              "         at least N times in the file -- for raw reads, where every sequencing error makes k-mers that occur\n"
              "         once; 1 = every sampled k-mer, the reference's set), --search_path auto|hits|topk [auto] (search:\n"
              "         topk selects the -n best per query on the device while blocks of the ANI matrix stream past -- memory\n"
              "         does not grow with the number of pairs above -a; hits builds the thresholded hit list first; auto =\n"
              "         topk for -n <= 64, hits beyond; both write the same file), --linkage single|greedy|setcover [single]\n"
              "         (cluster: greedy = one representative per cluster, as dereplication tools choose them -- a sketch is\n"
              "         a representative unless an earlier representative is within -a of it, else it joins the best such\n"
              "         one; representatives are pairwise below -a, every member is within -a of its own; one line per\n"
              "         sketch: file, cluster id, file of its representative, ANI with it -- 100 for a representative;\n"
              "         setcover = greedy set cover, as MMseqs2 and Linclust cluster: the sketch with the most still-uncovered\n"
              "         neighbours within -a becomes a representative and takes them as its members, ties to the first in\n"
              "         the file, until none is left -- the guarantees and the lines of greedy, the representative chosen by\n"
              "         coverage instead of file order; it holds the hits of the whole comparison, 12 bytes per pair within -a),\n"
              "         --order file|size [file] (cluster --linkage greedy: the order the sketches are processed in; size =\n"
              "         descending hv_norm_2, ties in file order -- the most complete genome of a group represents it;\n"
              "         cluster ids count the representatives in that order, the lines stay in file order),\n"
              "         --tree <file> (cluster --linkage single: the single-linkage tree at the floor -a -- the maximum-ANI\n"
              "         spanning forest, genomes - clusters lines, strongest first: file, file, ANI as dist prints it; cut\n"
              "         at any threshold >= -a it gives that threshold's clusters, its order is the merge order),\n"
              "         --levels L1,L2,... (cluster --linkage single: 1 to 8 further thresholds, ascending, above -a, all from\n"
              "         one comparison at -a; every line of -o becomes file, then for -a and each level the cluster id and\n"
              "         the file of the cluster's first member),\n"
              "         --columns LIST (dist: a comma list out of mash, containment, containment_ref, max_containment; every\n"
              "         line gets one further field per name, in the order listed -- the pair's ANI under that metric, whatever\n"
              "         --ani_metric selected the lines; containment_ref = the share of the reference's hashes found in the\n"
              "         query; runs on the first visible GPU),\n"
              "         --pairs FILE (dist: evaluate the pairs FILE lists, ref_name<TAB>qry_name[<TAB>anything] per line, names\n"
              "         as -r and -q carry them -- a dist TSV can be fed back; one line per listed pair in the order of the\n"
              "         list, ANI under --ani_metric, then the --columns fields; -a is not applied; runs on the first\n"
              "         visible GPU)\n");
}
void print_cluster_help() {
  print_help();
  std::printf("\ncluster --hclust average: average linkage (UPGMA), the hierarchical clustering of dRep and of scipy's\n"
              "         linkage(method=\"average\") on an ANI matrix, computed on the first visible GPU from the dense matrix of\n"
              "         all pairs (8 bytes per pair; up to 65536 sketches).  Every ANI counts as dist prints it, in thousandths:\n"
              "         the two clusters with the highest average ANI between their members merge, ties to the pair whose\n"
              "         first members come first in the file, while that average is at least -a [95.0].  -o gets the lines of\n"
              "         single linkage: file, cluster id, file of the cluster's first member.  --tree <file> writes the merges,\n"
              "         genomes - clusters lines, every child before its parent: file of the first member of the cluster that\n"
              "         stays, file of the first member of the one absorbed, average ANI of the merge as dist prints it, size\n"
              "         of the merged cluster.  It is a scheme of its own: it does not go with --linkage or --levels.\n");
  std::printf("\ncluster --agglomerate average|complete: the agglomerative clusterings on the dense matrix.  average is --hclust\n"
              "         average, the same files byte for byte.  complete is complete linkage, dRep's --clusterAlg complete and\n"
              "         scipy's linkage(method=\"complete\") on an ANI matrix (4 bytes per pair; up to 65536 sketches): the two\n"
              "         clusters whose least similar members have the highest ANI merge, ties to the pair whose first members\n"
              "         come first in the file, while that lowest ANI is at least -a [95.0] -- EVERY pair inside a cluster is at\n"
              "         least -a, as dist prints it, which no other scheme promises.  -o, --tree and --stats get the lines of\n"
              "         --hclust average; the third field of a --tree line is the lowest ANI between the two merged clusters.\n"
              "         It does not go with --hclust, --linkage or --levels.\n");
  std::printf("\ncluster --stats <file>: how good the clusters at -a are, with every --linkage and with --hclust, computed on the\n"
              "         first visible GPU from all pairs, block by block (no matrix is held).  Every ANI counts as dist prints\n"
              "         it, in thousandths.  One line per cluster, in id order: cluster id, size, file of the medoid (the member\n"
              "         with the highest sum of ANIs with the other members, ties to the one processed first), mean ANI within\n"
              "         the cluster over its ordered pairs, lowest ANI within the cluster -- far below -a: the cluster\n"
              "         chained --, files of the two members that have it, highest ANI between a member and a sketch outside,\n"
              "         file of that member, file of that sketch, cluster id of that sketch.  NA in the fields a singleton, or\n"
              "         a run with one cluster, does not have.  A cluster whose highest outside ANI is not below its lowest\n"
              "         within ANI is counted as not separated in the log.  -o is what it is without --stats.\n");
}

// `hyper-gen dist --help`: the general help with a paragraph on --newick behind it
void print_dist_help() {
  print_help();
  std::printf("\ndist --newick <file>: the neighbour-joining tree of all sketches of the one file -r and -q name, computed on the first\n"
              "         visible GPU from the dense matrix of all pairs (4 bytes per pair; up to 65536 sketches), whatever -a is.\n"
              "         The distance of a pair is 100 - ANI as dist prints it, in thousandths, held in fixed point (2^-15\n"
              "         thousandths); the rule is neighbour joining on integers: with c nodes left and r(i) the sum of a node's\n"
              "         distances, the pair with the lowest (c - 2) d(i, j) - r(i) - r(j) joins, ties to the pair whose first\n"
              "         members come first in the file, and the joined node is at (d(a, k) + d(b, k) - d(a, b)) / 2 from every\n"
              "         other k -- the tree depends on the ANI values alone and can be reproduced from a dist -a 0 TSV.  The\n"
              "         file is one line of Newick: every label is a name as the TSV carries it, in single quotes, a quote\n"
              "         inside doubled; the tree is unrooted, its top level has three children; branch lengths are substitutions\n"
              "         per site, 1 - ANI / 100, with eight decimals, and may be negative, as neighbour joining leaves them\n"
              "         (nothing is clamped).  -o is what it is without --newick.  It needs --ani_metric mash or\n"
              "         max_containment and does not go with --pairs or --shards.\n"
              "dist --fragments [--fragment_ani T] [--min_fragments N] [--fragment_hits FILE]: the ANI over the shared part of two\n"
              "         genomes and how much of them is shared, as FastANI, skani and GTDB's species rule (ANI >= 95 and aligned\n"
              "         fraction >= 0.5) report them.  -r and -q are sketch files written with sketch --fragment: consecutive\n"
              "         records whose names differ only in a final :start-end are the fragments of one genome, a record without\n"
              "         that suffix is a genome of one fragment, and a genome whose records are not consecutive is an error.\n"
              "         Every query fragment keeps its best window in every reference genome; it is matched when that ANI is at\n"
              "         least --fragment_ani T [90].  At the default -d 4096 the best of a genome's unrelated windows reads as an\n"
              "         ANI near 87 whatever -s is: fragment hits below about 88 are noise, keep T above that.  --ani_metric is\n"
              "         containment unless it is given: the share of the fragment's hashes found in the window.  One line per\n"
              "         (reference genome, query genome) with at least --min_fragments N [1] matched fragments and a genome ANI of\n"
              "         at least -a, ordered by query, then reference, in file order: reference, query, ANI, matched fragments,\n"
              "         all fragments of the query.  The ANI is the mean of the matched fragments' bests, every one counted as\n"
              "         dist prints it, in thousandths; the aligned fraction is matched / all.  With -r and -q naming one file\n"
              "         every ordered pair is written, a genome with itself too.  --fragment_hits FILE writes one line per matched\n"
              "         (reference genome, query fragment), ordered by query fragment, then reference genome: name of the\n"
              "         fragment, name of its best window, ANI.  It runs on the first visible GPU, block by block (no matrix is\n"
              "         held), and does not go with --pairs, --columns, --newick or --shards.\n");
  // (no blank line in front: everything behind the general help stays one block, as the --fragments text does)
  std::printf("dist --histogram FILE [--histogram_bin B]: how the ANI values of the WHOLE comparison are distributed -- the plot behind\n"
              "         the 95 %% species gap, and how many pairs a threshold will produce, known before it is run.  Every pair dist\n"
              "         enumerates is counted, whatever -a is: all of -r x -q with two files, the pairs i < j of one file, every\n"
              "         ordered pair i != j of one file under --ani_metric containment.  A value counts as dist prints it, in\n"
              "         thousandths; --histogram_bin B [0.1] is the width of a bin as an ANI, 0.001 to 100 with at most three\n"
              "         decimals (0.1: 1001 bins; 0.001: one bin per printed value).  FILE gets one line per bin, all bins,\n"
              "         ascending: the bin's first and last printed value, the pairs in it, the pairs in it and in all higher\n"
              "         bins.  That last field is the number of lines of a dist -a 0 TSV that PRINT at least the bin's first\n"
              "         value; it is not the number of lines dist -a x writes, which compares the unrounded value: a pair at\n"
              "         94.9996 prints 95.000 and fails -a 95.  The histogram is a second pass over the comparison on the first\n"
              "         visible GPU, block by block (no matrix is held; a width below 0.013 reads every block once per 8192 bins);\n"
              "         -o is what it is without --histogram.  It goes with --columns and --newick and does not go with --pairs,\n"
              "         --fragments or --shards.\n");
}

// `hyper-gen sketch --help`: the general help with a paragraph on --alphabet behind it
void print_sketch_help() {
  print_help();
  std::printf("\nsketch --alphabet dna|protein [dna]: protein sketches amino-acid k-mers, for genomes too far apart for nucleotide\n"
              "         k-mers (below roughly 80 %% identity two genomes share almost no 21-mers and every ANI reads 0): the AAI of\n"
              "         Mash -a, sourmash protein and Dashing 2 --protein.  The files are the *.faa of -p, plain or gzip: the\n"
              "         proteins of one genome each.  A residue is one of ACDEFGHIKLMNPQRSTVWY in either case (N is asparagine\n"
              "         here); a k-mer is -k consecutive residues of one record, 1 to 32, [9] when -k is not given (Mash's\n"
              "         protein default -- 21 residues would share nothing); one strand, no canonical choice.  The hash of a\n"
              "         k-mer is t1ha2 of its upper-cased bytes under -S, and -s samples it as it samples nucleotide k-mers;\n"
              "         -d is the hypervector's width.  The files go in batches through the first visible GPU.  The sketch\n"
              "         file has the layout of any other, its records carry -k and canonical = false: dist, search and\n"
              "         cluster read it as it is, and what they print is the AAI by the formula of the ANI.  Nothing in the file\n"
              "         says which alphabet it was made from: dist cannot tell a protein sketch file from a nucleotide one, and\n"
              "         comparing one with the other gives numbers that mean nothing.  It does not go with --min_count above 1,\n"
              "         with --shards or with -k above 32.  dna is what sketch does without the option.\n");
  std::printf("\nsketch --translate: sketches the amino-acid k-mers of all six reading frames of the nucleotide files of -p (the\n"
              "         files sketch reads anyway: *.fna, *.fa, *.fasta, plain or gzip), so that AAI needs no gene caller first:\n"
              "         sourmash's sketch translate.  It takes no value.  A base is one of ACGT in either case; codons translate\n"
              "         by the standard genetic code (NCBI table 1); a codon with any other byte in it (N, IUPAC codes) and a\n"
              "         stop end a k-mer, as a non-residue does under --alphabet protein.  Frames 1 to 3 start at the first,\n"
              "         second and third base, frames 4 to 6 are those of the reverse complement; a k-mer is -k consecutive\n"
              "         residues of one frame, 1 to 32, [9] when -k is not given; both strands contribute, no canonical choice.\n"
              "         The hash is the one --alphabet protein takes of the same residues, so the k-mers of a genome's called\n"
              "         proteins are a subset of its translated ones: dist --ani_metric containment of a protein sketch against\n"
              "         a translated one says whether those proteins are encoded in that assembly.  The files go in batches\n"
              "         through the first visible GPU; the records carry -k in residues and canonical = false, and dist, search\n"
              "         and cluster print the AAI.  It does not go with --alphabet protein (protein input is not translated),\n"
              "         with --min_count above 1, with --shards or with -k above 32.\n"
              "sketch --individual [--min_length N]: one sketch per FASTA record instead of one per file, for the collections that\n"
              "         come as one multi-FASTA -- plasmid and viral databases, the contigs of an assembly: Mash -i, sourmash\n"
              "         --singleton, skani -i.  It takes no value.  Every file of -p (plain or gzip, below 4 GiB inflated) goes to\n"
              "         the first visible GPU as it is and is split into its records there; the sketch parameters are those of\n"
              "         sketch without the option (-k up to 255, -s, -S, -C, --min_count, --pack_layout, -D).  A record starts at a\n"
              "         line that begins with '>'; its name in the sketch file is its identifier, the header up to the first\n"
              "         blank, without the file's path; files go in the order sketch reads them, records in file order.  Names\n"
              "         that repeat are kept, a record without an identifier and sequence in front of the first header are\n"
              "         errors.  --min_length N [0] leaves out the records with fewer than N sequence bytes; it needs --individual.\n"
              "         It does not go with --alphabet protein, with --translate or with --shards.\n"
              "sketch --fragment W [--fragment_step S]: one sketch per window of W bases of every file's merged sequence, a window\n"
              "         starting every S bases [W]: the fragments that dist --fragments compares, as FastANI and skani cut them.\n"
              "         W and S are multiples of 4, S is at most W and W at least -k.  A sequence of up to W bases is one window;\n"
              "         a last window shorter than W / 2 is dropped, which cannot happen with S up to W / 2.  Cut the query side\n"
              "         with --fragment L and the reference side with --fragment 2L --fragment_step L: every colinear stretch of L\n"
              "         bases then lies whole inside one reference window.  The name of a record is file:start-end, 1-based and\n"
              "         inclusive, in the merged sequence; everything else in it is what sketch writes.  Every file goes to the\n"
              "         first visible GPU once and its windows are sketched from that one copy.  It does not go with\n"
              "         --individual, with --alphabet protein, with --translate or with --shards.\n");
}

// `hyper-gen triangle --help`: the general help (which does not list the subcommand: its text is pinned) with a paragraph on
// the matrix file behind it
void print_triangle_help() {
  print_help();
  std::printf("hyper-gen triangle -p {sketch_file} -o {output_matrix} [-t N] [--ani_metric mash|max_containment|containment]: the ANI of\n"
              "         all pairs of the file's n sketches as a PHYLIP-like matrix of fixed-width text, formatted on the first\n"
              "         visible GPU block by block while the host writes the block before.  The first line is n; then one line per\n"
              "         sketch: its name as dist writes it, a tab, and the row's fields.  A field is 8 bytes: the ANI as dist\n"
              "         prints it, right-aligned in 7 characters (\"  0.000\", \" 95.123\", \"100.000\"), then a tab, or a newline\n"
              "         behind the row's last field.  --ani_metric mash [default] and max_containment write the lower triangle: row\n"
              "         i carries the fields j < i, row 0 its name alone, and the fields of row i start 8 * i * (i - 1) / 2 bytes\n"
              "         into the field text.  --ani_metric containment is directional and writes the square: row i carries all n\n"
              "         fields, the diagonal included, starting 8 * i * n bytes into the field text.  In the file the field (i, j)\n"
              "         lies at the length of the first line, plus the lengths of the names of rows 0..i and one byte each, plus\n"
              "         the start of row i in the field text, plus 8 * j: a reader can seek to any pair.  Every field equals the third\n"
              "         column of the same file's dist -a 0 line for that pair, so the matrix can be reproduced from dist -a 0.\n"
              "         -a is accepted and ignored: every pair is written.  -t threads [16] write a block's rows.\n");
}

// what --translate and --alphabet protein (`opt`; its input is `input`) have in common: neither goes with --min_count or
// --shards, k defaults to 9 and is at most 32
void amino_acid_mode(Cli &c, const std::string &opt, const std::string &input) {
  if (c.min_count > 1) die("--min_count is not supported with " + opt + ": amino-acid k-mers are sketched without the count filter");
  if (c.shards) die("--shards is not supported with " + opt + ": " + input + " input is sketched on the first visible GPU");
  if (!given(c, "ksize")) c.ksize = 9;
  if (c.ksize > 32) die("invalid value '" + std::to_string(c.ksize) + "' for '--ksize': " + opt + " takes k-mers of 1 to 32 residues");
}

Cli parse(int argc, char **argv) {
  if (argc < 2) die("usage: hyper-gen <sketch|dist|search|cluster> [options]   (see --help)");
  Cli c;
  c.mode = argv[1];
  if (c.mode == "--version" || c.mode == "-V") {
    std::printf("hyper-gen 0.0.1 (%s)\n", hg_version());
    std::exit(0);
  }
  if (c.mode == "--help" || c.mode == "-h") {
    print_help();
    std::exit(0);
  }
  static const char *const modes[] = {"sketch", "dist", "search", "cluster", "triangle"};
  unsigned k_mode = 0;
  for (unsigned k = 0; k < 5; ++k)
    if (c.mode == modes[k]) c.mode_bit = 1u << (k_mode = k);
  if (!c.mode_bit) die("unknown subcommand '" + c.mode + "'");
  if (c.mode_bit != SKETCH) c.method = "fracminhash";
  if (c.mode_bit == CLUSTER) c.ani_th = 95.0f;
  for (int i = 2; i < argc; ++i) {
    Arg a{argv[i], "", nullptr};
    static void (*const help_of[])() = {print_sketch_help, print_dist_help, nullptr, print_cluster_help, print_triangle_help};  // by subcommand; search has none
    if (help_of[k_mode] && (a.flag == "--help" || a.flag == "-h")) {
      help_of[k_mode]();
      std::exit(0);
    }
    const Option *o = nullptr;
    bool have_val = false;
    if (a.flag.rfind("--", 0) == 0) {
      std::string name = a.flag.substr(2);
      const size_t eq = name.find('=');
      if (eq != std::string::npos) a.val = name.substr(eq + 1), name = name.substr(0, eq), have_val = true;
      for (const Option &x : options)
        if (name == x.name) o = &x;
      if (!o) die("unexpected argument '" + a.flag + "'");
    } else if (a.flag.size() >= 2 && a.flag[0] == '-') {
      for (const Option &x : options)
        if (a.flag[1] == x.letter) o = &x;
      if (a.flag.size() > 2) a.val = a.flag.substr(a.flag[2] == '=' ? 3 : 2), have_val = true;
    } else {
      die("unexpected argument '" + a.flag + "'");
    }
    if (o && !o->take) {  // a switch
      if (have_val) die("unexpected argument '" + a.flag + "'");
      c.given.set((size_t)(o - options));
      continue;
    }
    if (!have_val) {
      if (i + 1 >= argc) die("a value is required for '" + a.flag + "'");
      a.val = argv[++i];
    }
    if (!o) die("unexpected argument '" + a.flag + "'");  // (an unknown letter: after its value, as ever)
    a.name = o->name;
    o->take(c, a);
    c.given.set((size_t)(o - options));
  }
  if (!c.shards) c.given.reset(option_row("shards"));  // --shards 0 is the default
  for (size_t k = 0; k < N_OPTIONS; ++k) {
    if (!c.given[k]) continue;
    const std::string f = std::string("--") + options[k].name;
    if (!(options[k].modes & c.mode_bit)) die(f + " is not supported by " + c.mode + ": " + options[k].why);
    if (options[k].why_shards && c.shards) die(f + " is not supported with --shards: " + options[k].why_shards);
  }
  // what an option needs of the others
  const bool translate = given(c, "translate"), individual = given(c, "individual"), fragments = given(c, "fragments");
  for (const char *of_fragments : {"fragment_ani", "min_fragments", "fragment_hits"})
    if (given(c, of_fragments) && !fragments) die(std::string("--") + of_fragments + " needs --fragments: without it dist compares whole sketches");
  if (c.search_path == SearchPath::topk && c.top_n > HG_SEARCH_TOPK_MAX)
    die("--search_path topk takes -n up to " + std::to_string(HG_SEARCH_TOPK_MAX) + " (larger -n goes through the hit list)");
  if (given(c, "agglomerate") && given(c, "hclust"))
    die("--agglomerate does not go with --hclust: both choose the clustering on the dense matrix (--agglomerate average is --hclust average)");
  if (given(c, "agglomerate") && given(c, "linkage"))
    die("--agglomerate does not go with --linkage: average and complete linkage are schemes of their own, not ones of --linkage's");
  if (given(c, "agglomerate") && given(c, "levels"))
    die("--levels is not supported with --agglomerate: it cuts the single-linkage tree, not the dendrogram of average or complete linkage");
  if (c.hclust_average && given(c, "linkage"))
    die("--hclust does not go with --linkage: average linkage is a scheme of its own, not one of --linkage's");
  if (c.hclust_average && given(c, "levels"))
    die("--levels is not supported with --hclust: it cuts the single-linkage tree, not the dendrogram of average linkage");
  if (given(c, "order") && c.mode_bit == CLUSTER && c.linkage == Linkage::setcover)
    die("--order is not supported by cluster --linkage setcover: the order the representatives are chosen in is the rule's own");
  if (given(c, "order") && !(c.mode_bit == CLUSTER && c.linkage == Linkage::greedy))
    die("--order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches");
  if ((given(c, "tree") || given(c, "levels")) && c.linkage != Linkage::single)
    die(std::string(given(c, "tree") ? "--tree" : "--levels") + " needs cluster --linkage single: " +
        (c.linkage == Linkage::greedy ? "greedy" : "set-cover") + " clusters are not nested and have no tree");
  if (given(c, "levels") && !(c.levels[0] > c.ani_th))
    die("invalid value for '--levels': every level must be above -a, the threshold the tree is built at");
  if (c.mode_bit == CLUSTER && c.ani_metric == HG_ANI_CONTAINMENT)
    die("--ani_metric containment is not supported by cluster: it is directional (mash | max_containment)");
  if (given(c, "newick") && c.path_r != c.path_q) die("--newick needs one sketch file: -r and -q must name the same file");
  if (given(c, "newick") && c.ani_metric == HG_ANI_CONTAINMENT)
    die("--ani_metric containment is not supported with --newick: it is directional (mash | max_containment)");
  if (given(c, "newick") && given(c, "pairs")) die("--pairs is not supported with --newick: the tree needs every pair, not the listed ones");
  if (translate) {
    if (c.protein) die("--translate is not supported with --alphabet protein: protein input is not translated");
    amino_acid_mode(c, "--translate", "translated");  // (k defaults as for --alphabet protein)
  }
  if (individual) {
    if (c.protein) die("--individual is not supported with --alphabet protein: protein input is sketched one file at a time");
    if (translate) die("--individual is not supported with --translate: translated input is sketched one file at a time");
    if (c.shards) die("--shards is not supported with --individual: the records are sketched on the first visible GPU");
  }
  if (given(c, "min_length") && !individual) die("--min_length needs --individual: without it sketch makes one sketch per file, whatever its length");
  if (c.protein) amino_acid_mode(c, "--alphabet protein", "protein");  // (Mash's protein default for k)
  if (given(c, "fragment_step") && !given(c, "fragment")) die("--fragment_step needs --fragment: without it sketch makes one sketch per file");
  if (given(c, "fragment")) {
    if (individual) die("--fragment is not supported with --individual: the windows are cut from a file's merged sequence, not from its records");
    if (c.protein) die("--fragment is not supported with --alphabet protein: protein input is sketched one file at a time");
    if (translate) die("--fragment is not supported with --translate: translated input is sketched one file at a time");
    if (c.shards) die("--shards is not supported with --fragment: the windows are sketched on the first visible GPU");
    if (!given(c, "fragment_step")) c.fragment_step = c.fragment;
    if (c.fragment == 0 || c.fragment % 4) die("invalid value '" + std::to_string(c.fragment) + "' for '--fragment': a window is a multiple of 4 bases, at least 4");
    if (c.fragment_step == 0 || c.fragment_step % 4)
      die("invalid value '" + std::to_string(c.fragment_step) + "' for '--fragment_step': a step is a multiple of 4 bases, at least 4");
    if (c.fragment_step > c.fragment) die("invalid value '" + std::to_string(c.fragment_step) + "' for '--fragment_step': a step above the window would leave bases out");
    if (c.fragment < c.ksize) die("invalid value '" + std::to_string(c.fragment) + "' for '--fragment': a window shorter than -k holds no k-mer");
  }
  if (given(c, "histogram_bin") && !given(c, "histogram")) die("--histogram_bin needs --histogram: without it dist counts no pairs");
  if (given(c, "histogram")) {
    if (given(c, "pairs")) die("--histogram is not supported with --pairs: it counts every pair of the comparison, not the listed ones");
    if (fragments) die("--histogram is not supported with --fragments: it counts the ANI of whole sketches, not of fragments");
  }
  if (fragments) {
    if (given(c, "pairs")) die("--pairs is not supported with --fragments: every pair of genomes is compared");
    if (given(c, "columns")) die("--columns is not supported with --fragments: a line carries the fragment ANI, the matched and the total fragments");
    if (given(c, "newick")) die("--newick is not supported with --fragments: the tree is drawn from whole sketches");
    if (c.shards) die("--shards is not supported with --fragments: it runs on the first visible GPU");
    if (!given(c, "ani_metric")) c.ani_metric = HG_ANI_CONTAINMENT;  // the share of a fragment found in its best window
  }
  return c;
}

void ck(hg_ctx *ctx, hg_status s, const char *what) {
  if (s != HG_OK) die(std::string(what) + ": " + hg_status_str(s) + " (" + hg_last_error(ctx) + ")");
}
void ckm(hg_multi *m, hg_status s, const char *what) {
  if (s != HG_OK) die(std::string(what) + ": " + hg_status_str(s) + " (" + hg_multi_last_error(m) + ")");
}

// every GPU the process can see (HIP_VISIBLE_DEVICES narrows it); the reference opens device 0 only
// (src/sketch_cuda.rs:52)
hg_multi *open_all_devices(unsigned shards) {
  const int n = hg_device_count();
  if (n <= 0) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  // (--shards N: N shards dealt round the devices -- repeated ids run several shards on one GPU, which is how the
  // several-GPU code path is exercised on a one-GPU box)
  std::vector<int> ids(shards ? shards : (unsigned)n);
  for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int)(i % (size_t)n);
  hg_multi *m = nullptr;
  if (hg_multi_create(ids.data(), (int)ids.size(), &m) != HG_OK) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  return m;
}

// get_fasta_files (src/utils.rs:208-221): *.fna, *.fa, *.fasta, in that order
std::vector<std::string> fasta_files(const std::string &dir, std::initializer_list<const char *> patterns = {"*.fna", "*.fa", "*.fasta"}) {
  std::vector<std::string> out;
  for (const char *pat : patterns) {
    glob_t g;
    std::string p = dir + (dir.empty() || dir.back() == '/' ? "" : "/") + pat;
    if (glob(p.c_str(), 0, nullptr, &g) == 0)
      for (size_t i = 0; i < g.gl_pathc; ++i) out.push_back(g.gl_pathv[i]);
    globfree(&g);
  }
  return out;
}

// ---- what the four sketch drivers share: the parameters, the records, the closing lines ---------------------------------
// --scaled and --hv_d checked, then the sketch parameters of the command line.  companion: --alphabet protein and --translate,
// which hash one strand and have no count filter.
hg_sketch_params sketch_params(const Cli &c, bool companion) {
  if (c.scaled == 0) die("scaled must be >= 1");
  if (c.hv_d == 0 || c.hv_d > 32768) die("hv_d must be in 1..32768");
  if (c.hv_d % 256)  // the reference packs whole 256-blocks only (src/hd.rs:147) and says nothing; same bytes here
    logline("WARN", "hv_d is not a multiple of 256: the dimensions behind the last whole block are lost in the .sketch file (as in the reference)");
  hg_sketch_params p;
  hg_sketch_params_default(&p);
  const bool gpu_mode = c.device == "gpu";
  p.ksize = c.ksize, p.scaled = c.scaled, p.seed = c.seed;
  // -C is honoured by the reference's CUDA kernel only (src/cuda_kernel.cu:312-314); its CPU path always takes
  // needletail's canonical_kmers (src/sketch.rs:89) -- the flag still goes into the .sketch records as given
  p.canonical = companion ? 0u : gpu_mode ? (c.canonical ? 1u : 0u) : 1u;
  p.hv_d = (uint32_t)c.hv_d, p.hv_layout = HG_LAYOUT_AVX2;
  p.norm_mode = companion || gpu_mode ? HG_NORM_ACGT : HG_NORM_U2T;
  p.min_count = companion ? 1 : c.min_count;
  return p;
}

// The records of a .sketch file while they are collected; they point into the names and payloads, which are owned here
// (deques: growing them moves no element).
struct SketchRecords {
  const Cli &c;
  std::deque<std::string> names;
  std::deque<std::vector<int16_t>> payload;
  std::vector<hg_file_sketch> recs;
  explicit SketchRecords(const Cli &cli, size_t n = 0) : c(cli), recs(n) {}
  // record `at` (recs.size(): one more) from a sketched row: the hypervector compressed, the rest from the command line
  void put(size_t at, const int16_t *hv, int32_t norm2, std::string name, bool canonical) {
    const uint32_t q = hg_hv_quant_bits(hv, (uint32_t)c.hv_d);  // if_compressed is hard-wired true (utils.rs:200)
    const size_t pk_bytes = c.pack_naive ? hg_hv_packed_bytes_naive((uint32_t)c.hv_d, q) : hg_hv_packed_bytes((uint32_t)c.hv_d, q);
    payload.emplace_back((pk_bytes + 1) / 2);  // (the i16 view of the bytes, src/hd.rs:155-157)
    if ((c.pack_naive ? hg_hv_pack_naive : hg_hv_pack)(hv, (uint32_t)c.hv_d, q, reinterpret_cast<uint8_t *>(payload.back().data())) != HG_OK) die("pack");
    names.push_back(std::move(name));
    if (at == recs.size()) recs.emplace_back();
    hg_file_sketch &r = recs[at];
    std::memset(&r, 0, sizeof r);
    r.ksize = (uint8_t)c.ksize, r.canonical = canonical, r.hv_quant_bits = (uint8_t)q, r.hv_norm_2 = norm2;
    r.scaled = c.scaled, r.seed = c.seed, r.hv_d = c.hv_d;
    r.file_str = names.back().c_str();
    r.hv = payload.back().data(), r.hv_len = pk_bytes / 2;  // align_to::<i16>().1: whole i16s
  }
};

// The closing lines of a sketch run started at t0: `head` ("Sketching N files") with the time and the speed in `unit`s, `note`
// if there is one, the .sketch file written, its size.
void finish_sketch(const Cli &c, double t0, const std::string &head, const char *unit, const SketchRecords &out, const std::string &note = "") {
  const size_t n = out.recs.size();
  const double secs = now_s() - t0;
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s took %.2fs - Speed: %.1f %s/s", head.c_str(), secs, n / std::max(secs, 1e-9), unit);
  logline("INFO", buf);
  if (!note.empty()) logline("INFO", note);
  if (hg_sketch_file_write(c.out.c_str(), out.recs.data(), n) != HG_OK) die("Dump sketch file failed!");
  size_t total = 8;
  for (auto &r : out.recs) total += 47 + std::strlen(r.file_str) + r.hv_len * 2;
  std::snprintf(buf, sizeof buf, "Dump sketch file to %s with size %.2f MB", c.out.c_str(), total / 1024.0 / 1024.0);
  logline("INFO", buf);
}

int run_sketch_batches(const Cli &c, const std::vector<std::string> &files);
int run_sketch_individual(const Cli &c, const std::vector<std::string> &files);
int run_sketch_fragments(const Cli &c, const std::vector<std::string> &files);

int run_sketch(const Cli &c) {
  if (c.path == "1" && c.out.empty()) die("the following required arguments were not provided: --path --out");
  if (c.out.empty()) die("the following required arguments were not provided: --out");
  if (c.protein) return run_sketch_batches(c, fasta_files(c.path, {"*.faa"}));
  if (given(c, "translate")) return run_sketch_batches(c, fasta_files(c.path));
  if (given(c, "individual")) return run_sketch_individual(c, fasta_files(c.path));
  if (given(c, "fragment")) return run_sketch_fragments(c, fasta_files(c.path));
  const auto files = fasta_files(c.path);
  const size_t n = files.size();
  logline("INFO", "Start sketching...");
  const double t0 = now_s();
  const hg_sketch_params p = sketch_params(c, false);
  const uint32_t read_mode = c.device == "gpu" ? HG_READ_MERGE : HG_READ_NEEDLETAIL;
  SketchRecords out(c, n);

  // Reader side: -t persistent threads pull file indices from one counter; every thread owns S page-locked buffers
  // and fills them round robin (hg_read_fastx_pinned: the device then fetches the sequence by DMA at the PCIe rate
  // -- malloc'ed buffers went through the runtime's bounce buffer at a quarter of it), pushing each genome into the
  // sketch stream.  A thread waits when its S buffers are all in flight, so the page-locked footprint stays at T*S
  // genomes however many files there are (locking pages costs ~0.25 ms per MB) and after its first S files no
  // thread allocates.  The buffers are per thread on purpose: a ring shared by all readers made every file land in
  // memory last written on another core complex or socket -- 2x (16 threads) to 5x (32) slower reads on the
  // 2-socket host.
  // Device side: hg_sketch_stream (one uploader + one compute thread per visible GPU, genomes go to the least
  // loaded one: SURVEY.md 8e, no exchange); this thread collects the results, which arrive in completion order
  // and are stored by file index.
  const size_t T = std::max<size_t>(1, std::min<size_t>(c.threads, std::max<size_t>(n, 1)));
  const size_t S = std::max<size_t>(4, (64 + T - 1) / T);
  struct Slot {
    uint8_t *p = nullptr;
    size_t cap = 0, len = 0;
    bool busy = false;  // pushed, result not collected yet
  };
  std::vector<Slot> slots(T * S);
  std::vector<Slot *> slot_of(n, nullptr);
  std::mutex mu;
  std::condition_variable cv_stream;
  std::vector<std::condition_variable> cv_space(T);  // one per reader: a result wakes the reader that owns the buffer, not all sixteen
  hg_sketch_stream *stream = nullptr;
  std::atomic<size_t> next{0};
  std::atomic<uint64_t> read_ns{0};
  std::vector<int> dev_node;
  // 2-bit packing (hg_pack2: 3 bits per base over the link) costs a reader ~0.3 ms per 5 Mbp and only pays when
  // the link is what limits, so every reader decides per file: if at least two of its own buffers are still in
  // flight when it starts on a file, the device side lags behind the readers -> pack this one.
  std::atomic<size_t> n_packed{0};
  const uint32_t pack_flags = HG_READ_PACK2 | (p.norm_mode == HG_NORM_U2T ? HG_READ_PACK2_U2T : 0u);
  auto reader = [&](size_t tid) {
    // Reader thread -> the CPUs of the NUMA node its device hangs off (the thread's page-locked buffers lie there wherever
    // the thread runs: filling and packing them from that socket is ~1.5x faster, and the DMA engine fetches them ~25 %
    // faster than from the other one).  Best effort.
    (void)hg_bind_thread_to_numa_node(dev_node[tid % dev_node.size()], (unsigned)T);
    size_t k = 0;
    for (size_t i; (i = next.fetch_add(1)) < n; k = (k + 1) % S) {
      Slot &sl = slots[tid * S + k];
      bool pack;
      {
        std::unique_lock<std::mutex> lk(mu);
        size_t in_flight = 0;
        for (size_t q = 0; q < S; ++q) in_flight += slots[tid * S + q].busy ? 1 : 0;
        pack = in_flight >= 2;
        cv_space[tid].wait(lk, [&] { return !sl.busy; });
      }
      const double tr0 = now_s();
      if (hg_read_fastx_pinned(files[i].c_str(), read_mode | (pack ? pack_flags : 0u), &sl.p, &sl.cap, &sl.len) != HG_OK)
        die("Opening .fna files failed: " + files[i]);
      read_ns.fetch_add((uint64_t)((now_s() - tr0) * 1e9));
      if (pack) n_packed.fetch_add(1);
      {
        std::unique_lock<std::mutex> lk(mu);
        sl.busy = true, slot_of[i] = &sl;
        cv_stream.wait(lk, [&] { return stream != nullptr; });  // the devices are opened while the first files are read
      }
      const hg_status ps = pack ? hg_sketch_stream_push_packed(stream, sl.p, sl.len, i) : hg_sketch_stream_push(stream, sl.p, sl.len, i);
      if (ps != HG_OK) die(std::string("sketch: ") + hg_sketch_stream_last_error(stream));
    }
  };
  const double td0 = now_s();
  const int nd = hg_device_count();  // (brings the HIP runtime up: the readers' page-locked buffers need it too)
  if (nd <= 0) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  for (int i = 0; i < nd; ++i) dev_node.push_back(hg_device_numa_node(i));
  std::vector<std::thread> readers;
  for (size_t t = 0; t < T && n; ++t) readers.emplace_back(reader, t);
  {
    std::vector<int> ids(nd);
    for (int i = 0; i < nd; ++i) ids[i] = i;
    hg_sketch_stream *st = nullptr;
    if (hg_sketch_stream_open(ids.data(), nd, &p, &st) != HG_OK) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
    debugf("%d device(s) opened in %.1f ms", nd, (now_s() - td0) * 1e3);
    std::lock_guard<std::mutex> lk(mu);
    stream = st;
    cv_stream.notify_all();
  }
  std::vector<int16_t> hv(c.hv_d);
  double t_wait = 0, t_pack = 0;
  for (size_t done = 0; done < n; ++done) {
    uint64_t f = 0;
    int32_t n2 = 0;
    uint32_t nh = 0;
    int got = 0;
    const double tw0 = now_s();
    if (hg_sketch_stream_pop(stream, &f, hv.data(), &n2, &nh, &got) != HG_OK || !got)
      die(std::string("sketch: ") + hg_sketch_stream_last_error(stream));
    size_t owner;
    {
      std::lock_guard<std::mutex> lk(mu);
      slot_of[f]->busy = false;  // the sequence is not needed any more
      owner = (size_t)(slot_of[f] - slots.data()) / S;
    }
    cv_space[owner].notify_one();
    const double ts1 = now_s();
    out.put(f, hv.data(), n2, files[f], c.canonical);
    t_wait += ts1 - tw0, t_pack += now_s() - ts1;
  }
  for (auto &t : readers) t.join();
  if (debug_log()) {
    double st[6];
    for (int e = 0; hg_sketch_stream_stats(stream, e, st) == HG_OK; ++e)
      debugf("device engine %d: uploader idle %.1f ms, waiting for a chunk %.1f ms, in copy calls %.1f ms; compute idle "
             "%.1f ms, busy %.1f ms; %.0f chunks", e, st[0] * 1e3, st[1] * 1e3, st[2] * 1e3, st[3] * 1e3, st[4] * 1e3, st[5]);
  }
  debugf("collector: waited %.1f ms for results, sketch compression %.1f ms; readers: %.2f ms per file and thread, "
         "%zu of %zu files sent 2-bit packed", t_wait * 1e3, t_pack * 1e3, n ? read_ns.load() / 1e6 / n : 0.0,
         n_packed.load(), n);
  finish_sketch(c, t0, "Sketching " + std::to_string(n) + " files", "files", out);
  const double tf0 = now_s();
  hg_sketch_stream_close(stream);
  for (auto &sl : slots) hg_pinned_free(sl.p);
  debugf("released buffers and devices in %.1f ms", (now_s() - tf0) * 1e3);
  return 0;
}

// fn(0) .. fn(n - 1) side by side: fn(0) on this thread, a thread each for the others
template <class F>
void parallel(size_t n, F fn) {
  std::vector<std::thread> th;
  for (size_t t = 1; t < n; ++t) th.emplace_back([&fn, t] { fn(t); });
  fn(0);
  for (auto &t : th) t.join();
}

// sketch --alphabet protein and sketch --translate: the files in batches of up to 256 files or 1 GB of sequence -- reader
// threads fill the batch (the *.faa files through hg_aa_read_fasta; the nucleotide files through the reader run_sketch uses),
// hg_aa_sketch_batch or hg_tx_sketch_batch sketches it on the first visible GPU.  Log lines, records and payloads are
// run_sketch's; the records carry canonical = false.
int run_sketch_batches(const Cli &c, const std::vector<std::string> &files) {
  const bool tx = given(c, "translate");
  const uint32_t read_mode = c.device == "gpu" ? HG_READ_MERGE : HG_READ_NEEDLETAIL;  // (run_sketch's choice)
  const size_t n = files.size();
  logline("INFO", "Start sketching...");
  const double t0 = now_s();
  const hg_sketch_params p = sketch_params(c, true);
  if (hg_device_count() <= 0) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  hg_ctx *ctx = nullptr;
  if (hg_ctx_create(0, &ctx) != HG_OK) die(std::string("no MI355X device: ") + hg_last_error(nullptr));

  SketchRecords out(c, n);
  constexpr size_t BATCH_FILES = 256, BATCH_BYTES = (size_t)1 << 30;
  struct Buf {
    uint8_t *p = nullptr;
    size_t cap = 0, len = 0;
  };
  std::vector<Buf> bufs(std::min(BATCH_FILES, n));
  const size_t T = std::max<size_t>(1, std::min<size_t>(c.threads, bufs.size()));
  std::vector<int16_t> hv;
  std::vector<int32_t> n2(bufs.size());
  std::vector<uint32_t> nh(bufs.size());
  std::vector<const uint8_t *> ptrs(bufs.size());
  std::vector<size_t> lens(bufs.size());
  for (size_t i0 = 0; i0 < n;) {
    // readers: a counter hands out the batch's buffers; the batch closes at BATCH_FILES files or once BATCH_BYTES are read
    std::atomic<size_t> next{0}, bytes{0};
    parallel(T, [&](size_t) {
      for (size_t k; bytes.load() < BATCH_BYTES && (k = next.fetch_add(1)) < bufs.size() && i0 + k < n;) {
        Buf &b = bufs[k];
        const char *path = files[i0 + k].c_str();
        const hg_status rs = tx ? hg_read_fastx_into(path, read_mode, &b.p, &b.cap, &b.len) : hg_aa_read_fasta(path, &b.p, &b.cap, &b.len);
        if (rs != HG_OK) die(std::string("Opening ") + (tx ? ".fna" : ".faa") + " files failed: " + files[i0 + k]);
        bytes.fetch_add(b.len);
      }
    });
    // (the counter may have run past the files that were read: the batch is the files handed out, which are consecutive)
    const size_t m = std::min({next.load(), bufs.size(), n - i0});
    for (size_t k = 0; k < m; ++k) ptrs[k] = bufs[k].p, lens[k] = bufs[k].len;
    hv.resize(m * c.hv_d);
    ck(ctx, (tx ? hg_tx_sketch_batch : hg_aa_sketch_batch)(ctx, ptrs.data(), lens.data(), m, &p, hv.data(), n2.data(), nh.data()), "sketch");
    for (size_t k = 0; k < m; ++k) out.put(i0 + k, hv.data() + k * c.hv_d, n2[k], files[i0 + k], false);
    i0 += m;
  }
  finish_sketch(c, t0, "Sketching " + std::to_string(n) + " files", "files", out);
  for (Buf &b : bufs) hg_free(b.p);
  hg_ctx_destroy(ctx);
  return 0;
}

// One hg_dev_alloc allocation of n elements of T, freed with the object
template <class T>
class DevBuf {
  hg_ctx *ctx;
  T *p = nullptr;

 public:
  explicit DevBuf(hg_ctx *c) : ctx(c) {}  // (empty: alloc() or a move fills it)
  DevBuf(hg_ctx *c, size_t n) : ctx(c) { alloc(n); }
  DevBuf &operator=(DevBuf &&o) noexcept { return std::swap(ctx, o.ctx), std::swap(p, o.p), *this; }
  ~DevBuf() { if (p) (void)hg_dev_free(ctx, p); }
  void alloc(size_t n) {  // (what it held is freed first)
    if (p) ck(ctx, hg_dev_free(ctx, release()), "free");
    void *v = nullptr;
    ck(ctx, hg_dev_alloc(ctx, n * sizeof(T), &v), "alloc");
    p = static_cast<T *>(v);
  }
  T *get() const { return p; }
  T *release() { return std::exchange(p, nullptr); }  // (the caller frees it)
  void upload(const T *host, size_t n) { ck(ctx, hg_copy_h2d(ctx, p, host, n * sizeof(T)), "upload"); }
  void download(T *host, size_t n) const { ck(ctx, hg_copy_d2h(ctx, host, p, n * sizeof(T)), "download"); }
};

// sketch --individual: every file goes to the first visible GPU as text (hg_rec_read_text: gzip inflated, page-locked),
// hg_rec_sketch_text_dev splits it into its records there and sketches them in sub-batches, and the rows come back through
// take_rows, which packs them.  The parameters are run_sketch's; a record's file_str is its identifier.
struct IndividualRows {
  const std::string *file;
  const uint8_t *text;
  SketchRecords out;
};
int take_rows(void *user, const hg_rec_entry *table, size_t n_recs, const uint32_t *which, size_t m, const int16_t *hv, const int32_t *n2,
              const uint32_t *) {
  IndividualRows &o = *static_cast<IndividualRows *>(user);
  const Cli &c = o.out.c;
  if (m == 0) {  // the table alone: every record must have a name, also one that --min_length leaves out
    for (size_t r = 0; r < n_recs; ++r)
      if (!table[r].id_len) die(*o.file + ": record " + std::to_string(r + 1) + " has an empty identifier");
    return 0;
  }
  for (size_t k = 0; k < m; ++k) {
    const hg_rec_entry &e = table[which[k]];
    o.out.put(o.out.recs.size(), hv + k * c.hv_d, n2[k], std::string(reinterpret_cast<const char *>(o.text + e.hdr_off + 1), e.id_len),
              c.canonical);
  }
  return 0;
}

int run_sketch_individual(const Cli &c, const std::vector<std::string> &files) {
  logline("INFO", "Start sketching...");
  const double t0 = now_s();
  const hg_sketch_params p = sketch_params(c, false);  // (run_sketch's reading of -C and -D)
  if (hg_device_count() <= 0) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  hg_ctx *ctx = nullptr;
  if (hg_ctx_create(0, &ctx) != HG_OK) die(std::string("no MI355X device: ") + hg_last_error(nullptr));

  IndividualRows rows{nullptr, nullptr, SketchRecords(c)};
  uint8_t *text = nullptr;
  size_t cap = 0, n_total = 0;
  for (const std::string &file : files) {
    size_t n = 0;
    const hg_status rs = hg_rec_read_text(file.c_str(), &text, &cap, &n);
    if (rs == HG_ERR_UNSUPPORTED) die(file + ": the file holds 2^32 bytes or more after inflation, --individual takes files below 4 GiB");
    if (rs != HG_OK) die("Opening .fna files failed: " + file);
    DevBuf<uint8_t> d_text(ctx, ((n + 15) & ~(size_t)15) + 16);
    d_text.upload(text, n);
    rows.file = &file, rows.text = text;
    size_t n_recs = 0, n_kept = 0;
    const hg_status ss = hg_rec_sketch_text_dev(ctx, d_text.get(), n, &p, c.min_length, take_rows, &rows, &n_recs, &n_kept);
    if (ss != HG_OK) die(file + ": " + hg_status_str(ss) + " (" + hg_last_error(ctx) + ")");
    debugf("%s: %zu bytes, %zu records, %zu sketched", file.c_str(), n, n_recs, n_kept);
    n_total += n_recs;
  }
  hg_pinned_free(text);
  const size_t n = rows.out.recs.size();
  char note[128] = "";
  if (n < n_total) std::snprintf(note, sizeof note, "%zu records shorter than %llu were left out", n_total - n, c.min_length);
  finish_sketch(c, t0, "Sketching " + std::to_string(n) + " records of " + std::to_string(files.size()) + " files", "records", rows.out, note);
  hg_ctx_destroy(ctx);
  return 0;
}

// sketch --fragment W [--fragment_step S]: every file's merged sequence goes to the first visible GPU once (the reader and
// the parameters are run_sketch's), hg_frag_sketch_seq_dev sketches its windows from that one copy in sub-batches, and the
// rows come back through take_windows, which packs them.  A record's file_str is file:start-end, 1-based and inclusive.
struct FragmentRows {
  const std::string *file;
  SketchRecords out;
};
int take_windows(void *user, const uint64_t *starts, const uint64_t *lens, size_t, size_t m, const int16_t *hv, const int32_t *n2, const uint32_t *) {
  FragmentRows &o = *static_cast<FragmentRows *>(user);
  const Cli &c = o.out.c;
  for (size_t k = 0; k < m; ++k)
    o.out.put(o.out.recs.size(), hv + k * c.hv_d, n2[k], *o.file + ":" + std::to_string(starts[k] + 1) + "-" + std::to_string(starts[k] + lens[k]),
              c.canonical);
  return 0;
}

int run_sketch_fragments(const Cli &c, const std::vector<std::string> &files) {
  logline("INFO", "Start sketching...");
  const double t0 = now_s();
  const hg_sketch_params p = sketch_params(c, false);  // (run_sketch's reading of -C and -D)
  const uint32_t read_mode = c.device == "gpu" ? HG_READ_MERGE : HG_READ_NEEDLETAIL;
  if (hg_device_count() <= 0) die(std::string("no MI355X device: ") + hg_last_error(nullptr));
  hg_ctx *ctx = nullptr;
  if (hg_ctx_create(0, &ctx) != HG_OK) die(std::string("no MI355X device: ") + hg_last_error(nullptr));

  FragmentRows rows{nullptr, SketchRecords(c)};
  uint8_t *seq = nullptr;
  size_t cap = 0;
  for (const std::string &file : files) {
    size_t n = 0;
    if (hg_read_fastx_pinned(file.c_str(), read_mode, &seq, &cap, &n) != HG_OK) die("Opening .fna files failed: " + file);
    DevBuf<uint8_t> d_seq(ctx, ((n + 3) & ~(size_t)3) + 64);  // (the 32 readable bytes behind the genome, and room for a whole last dword)
    if (n) d_seq.upload(seq, n);
    rows.file = &file;
    size_t n_windows = 0;
    const hg_status ss = hg_frag_sketch_seq_dev(ctx, d_seq.get(), n, &p, c.fragment, c.fragment_step, take_windows, &rows, &n_windows);
    if (ss != HG_OK) die(file + ": " + hg_status_str(ss) + " (" + hg_last_error(ctx) + ")");
    debugf("%s: %zu bases, %zu windows", file.c_str(), n, n_windows);
  }
  hg_pinned_free(seq);
  finish_sketch(c, t0, "Sketching " + std::to_string(rows.out.recs.size()) + " windows of " + std::to_string(files.size()) + " files", "windows", rows.out);
  hg_ctx_destroy(ctx);
  return 0;
}

// A loaded .sketch file: the records (names, norms, widths) on the host, the bit-packed payloads still inside the file
// image.  decompress_file_sketch (src/hd.rs:171-180) happens on the device: the image's payload bytes go over the link as
// they are (4.6 KB per sketch at 9 bits against 8 KB of int16) and hg_hv_unpack_batch_dev decodes them into the matrix
// the dist kernels read -- no host unpack threads, no second copy of the matrix in host memory.
struct Loaded {
  hg_sketch_file *f = nullptr;
  std::vector<int32_t> n2;
  std::vector<uint64_t> off;     // payload offsets in the image
  std::vector<uint8_t> q, lay;   // quantisation bits, payload layout (BitPacker8x / the non-AVX2 one) per record
  std::vector<uint32_t> len;     // strlen of the record's file_str: looked up once per file, not once per output line
  size_t n = 0;
  uint64_t hv_d = 0;
  uint8_t ksize = 0;
  size_t put_name(char *w, size_t i) const {  // record i's file_str at w
    std::memcpy(w, hg_sketch_file_get(f, i)->file_str, len[i]);
    return len[i];
  }
};

void load(const std::string &path, Loaded &L) {
  logline("INFO", "Loading sketch from " + path);
  if (hg_sketch_file_read_image(path.c_str(), &L.f) != HG_OK) die("Opening sketch file failed!");
  L.n = hg_sketch_file_count(L.f);
  if (L.n == 0) die("empty sketch file " + path);
  const hg_file_sketch *r0 = hg_sketch_file_get(L.f, 0);
  L.hv_d = r0->hv_d, L.ksize = r0->ksize;
  // validate before sizing anything from the file's own numbers
  if (L.hv_d == 0 || L.hv_d > 65536) die("unsupported HV dimension in " + path);
  L.n2.resize(L.n), L.off.resize(L.n), L.q.resize(L.n), L.lay.resize(L.n), L.len.resize(L.n);
  for (size_t i = 0; i < L.n; ++i) {
    const hg_file_sketch *r = hg_sketch_file_get(L.f, i);
    if (r->hv_quant_bits < 1 || r->hv_quant_bits > 16) die("corrupt sketch record (quantisation bits) in " + path);
    if (r->hv_d != L.hv_d) die("sketches of one file use different HV dimensions");
    // which of the reference's two payload layouts this is follows from its length (they never coincide)
    const int lay = hg_hv_payload_layout((uint32_t)L.hv_d, r->hv_quant_bits, (size_t)r->hv_len * 2);
    if (lay < 0) die("corrupt sketch payload in " + path);
    L.n2[i] = r->hv_norm_2, L.off[i] = hg_sketch_file_payload_offset(L.f, i), L.q[i] = r->hv_quant_bits, L.lay[i] = (uint8_t)lay;
    L.len[i] = (uint32_t)std::strlen(r->file_str);
  }
}

// The sketches of a file on the devices: shard s (hg_shard_range) gets the slice of the file image that holds its
// records, decodes it there and keeps the int16 rows and the norms (what hg_dist_multi_dev takes).
struct DevSet {
  std::vector<const int16_t *> hv;
  std::vector<const int32_t *> n2;
  std::vector<size_t> rows;
};
// whole: every shard gets ALL records (the query side of the top-k search: the small side is broadcast).
// perm (one shard only; cluster --order): row k of the matrix is record perm[k] -- the decode offsets are permuted, the
// payload bytes travel as they lie in the file.
void to_devices(hg_multi *m, const Loaded &L, DevSet &D, bool whole = false, const std::vector<uint32_t> *perm = nullptr) {
  char buf[96];
  std::snprintf(buf, sizeof buf, "Decompressing sketch with HV dim=%llu", (unsigned long long)L.hv_d);
  logline("INFO", buf);
  const int ns = hg_multi_size(m);
  D.hv.assign(ns, nullptr), D.n2.assign(ns, nullptr), D.rows.assign(ns, 0);
  size_t img_bytes = 0;
  const uint8_t *img = hg_sketch_file_image(L.f, &img_bytes);
  parallel((size_t)ns, [&](size_t s) {
    size_t lo = 0, hi = 0;
    hg_shard_range(L.n, (int)s, ns, &lo, &hi);
    if (whole) lo = 0, hi = L.n;
    if (hi == lo) return;
    hg_ctx *ctx = hg_multi_ctx(m, (int)s);
    const uint64_t b0 = L.off[lo], b1 = L.off[hi - 1] + 2 * hg_sketch_file_get(L.f, hi - 1)->hv_len;
    if (b1 > img_bytes || b0 > b1) die("corrupt sketch payload");
    std::vector<uint64_t> rel(hi - lo);
    for (size_t i = lo; i < hi; ++i) rel[i - lo] = L.off[i] - b0;
    std::vector<int32_t> p_n2;
    std::vector<uint8_t> p_q, p_lay;
    if (perm) {
      if (ns != 1 || perm->size() != L.n) die("internal: a permuted upload takes one shard and every record");
      p_n2.resize(L.n), p_q.resize(L.n), p_lay.resize(L.n);
      for (size_t k = 0; k < L.n; ++k) {
        const uint32_t i = (*perm)[k];
        rel[k] = L.off[i] - b0, p_n2[k] = L.n2[i], p_q[k] = L.q[i], p_lay[k] = L.lay[i];
      }
    }
    const int32_t *n2_src = perm ? p_n2.data() : L.n2.data() + lo;
    const uint8_t *q_src = perm ? p_q.data() : L.q.data() + lo, *lay_src = perm ? p_lay.data() : L.lay.data() + lo;
    DevBuf<uint8_t> d_img(ctx, b1 - b0);
    DevBuf<int16_t> d_hv(ctx, (hi - lo) * L.hv_d);
    DevBuf<int32_t> d_n2(ctx, hi - lo);
    d_img.upload(img + b0, b1 - b0);
    d_n2.upload(n2_src, hi - lo);
    ck(ctx, hg_hv_unpack_batch_dev(ctx, d_img.get(), b1 - b0, rel.data(), q_src, lay_src, hi - lo, (uint32_t)L.hv_d, d_hv.get()), "unpack");
    D.hv[s] = d_hv.release(), D.n2[s] = d_n2.release(), D.rows[s] = hi - lo;
  });
}
void release(hg_multi *m, DevSet &D) {
  for (size_t s = 0; s < D.hv.size(); ++s) {
    hg_ctx *ctx = hg_multi_ctx(m, (int)s);
    if (D.hv[s]) (void)hg_dev_free(ctx, const_cast<int16_t *>(D.hv[s]));
    if (D.n2[s]) (void)hg_dev_free(ctx, const_cast<int32_t *>(D.n2[s]));
  }
}

// "{:.3}" of an ANI (0 <= ani <= 100, src/utils.rs:277-282) without snprintf: ani * 1000 is exact in a double (24-bit
// significand times a 10-bit integer), so rounding that product to the nearest integer, ties to even (rint under the
// default rounding mode), is the correctly rounded decimal -- what Rust's exact-mode float formatting and glibc's %.3f
// both print.  Ties exist (ani = odd / 16: about one f32 in 16 000 near 96) and round-half-up would print 400 of the 1.1e9
// floats in [0, 100] differently: checked exhaustively against 128-bit integer arithmetic.  Writes "\t<int>.<3 digits>\n".
// (The library clamps ANI to [0, 100] -- src/dist.rs:156-159 -- so at most 3 + 1 + 3 digits follow the tab: the callers
// reserve 10 bytes per line for this.  The bound must not hang on another translation unit's arithmetic: anything that is
// not a number in [0, 100] -- a NaN, a negative value, a corrupted hit -- is brought into the range here.)
inline size_t put_ani(char *o, float ani) {
  if (!(ani >= 0.0f)) ani = 0.0f;  // NaN too
  if (ani > 100.0f) ani = 100.0f;
  const uint64_t v = (uint64_t)__builtin_rint((double)ani * 1000.0);
  uint64_t ip = v / 1000;
  const uint32_t fp = (uint32_t)(v % 1000);
  char tmp[24];
  size_t n = 0;
  do tmp[n++] = (char)('0' + ip % 10), ip /= 10;
  while (ip);
  size_t k = 0;
  o[k++] = '\t';
  while (n) o[k++] = tmp[--n];
  o[k++] = '.', o[k++] = (char)('0' + fp / 100), o[k++] = (char)('0' + fp / 10 % 10), o[k++] = (char)('0' + fp % 10), o[k++] = '\n';
  return k;
}

// An uninitialised array of hits (a std::vector would zero -- and so touch -- every page of a capacity-sized buffer of
// which a comparison fills one part in sixteen)
struct HitBuf {
  hg_ani_hit *p = nullptr;
  size_t n = 0;
  ~HitBuf() { std::free(p); }
  void resize(size_t m) {
    std::free(p);
    p = static_cast<hg_ani_hit *>(std::malloc(std::max<size_t>(m, 1) * sizeof(hg_ani_hit)));
    if (!p) die("out of memory");
    n = m;
  }
};

// All pairs with ANI >= ani_th of (R x Q) -- or of R against itself, i < j, when Q == nullptr --, on the host.  `order`:
// in dump_ani_file's order (src/utils.rs:262-269).  With one device the hits stay there until they are ordered (dist ->
// radix passes -> one download); with several, the shards' lists meet on the host and go through device 0 for the order.
// d_keep != nullptr: the list is wanted on device 0 (for hg_topk_per_query_dev), not on the host: *d_keep receives it
// and `hits` stays empty.
size_t all_hits(hg_multi *multi, const Loaded &R, const DevSet &dR, const Loaded *Q, const DevSet *dQ, float ani_th, bool order,
                HitBuf &hits, DevBuf<hg_ani_hit> *d_keep = nullptr) {
  const bool sym = Q == nullptr;
  const size_t qn = sym ? R.n : Q->n, total = sym ? R.n * (R.n - 1) / 2 : R.n * qn;
  size_t cap = std::max<size_t>(1024, total / 16), found = 0;
  const double t_in = now_s();
  hg_ctx *ctx = hg_multi_ctx(multi, 0);
  if (hg_multi_size(multi) == 1) {
    DevBuf<hg_ani_hit> d_hits(ctx);
    for (;;) {
      d_hits.alloc(cap);
      const hg_status s = hg_dist_dev(ctx, dR.hv[0], dR.n2[0], R.n, sym ? dR.hv[0] : dQ->hv[0], sym ? dR.n2[0] : dQ->n2[0], qn,
                                      (uint32_t)R.hv_d, R.ksize, sym, ani_th, d_hits.get(), cap, &found);
      if (s != HG_ERR_CAPACITY) {
        ck(ctx, s, "dist");
        break;
      }
      cap = found;
    }
    const double t1 = now_s();
    if (order) ck(ctx, hg_sort_ani_hits_dev(ctx, d_hits.get(), found, qn), "sort");
    if (d_keep) {
      *d_keep = std::move(d_hits);
      debugf("  dist on the device %.1f ms", (t1 - t_in) * 1e3);
      return found;
    }
    if (order) ck(ctx, hg_ctx_sync(ctx), "sort");
    const double t2 = now_s();
    hits.resize(found);
    if (found) d_hits.download(hits.p, found);
    debugf("  dist on the device %.1f ms, order %.1f ms, download %.1f ms", (t1 - t_in) * 1e3, (t2 - t1) * 1e3, (now_s() - t2) * 1e3);
    return found;
  }
  for (;;) {
    hits.resize(cap);
    // reference rows are all-gathered over xGMI, query rows stay on their shard's GPU
    const hg_status s = hg_dist_multi_dev(multi, dR.hv.data(), dR.n2.data(), dR.rows.data(), sym ? nullptr : dQ->hv.data(),
                                          sym ? nullptr : dQ->n2.data(), sym ? nullptr : dQ->rows.data(), (uint32_t)R.hv_d, R.ksize,
                                          sym, ani_th, hits.p, cap, &found);
    if (s != HG_ERR_CAPACITY) {
      ckm(multi, s, "dist");
      break;
    }
    cap = found;
  }
  hits.n = found;
  if (order) ck(ctx, hg_sort_ani_hits_staged(ctx, hits.p, found, qn), "sort");
  if (d_keep) {
    *d_keep = DevBuf<hg_ani_hit>(ctx, std::max<size_t>(found, 1));
    if (found) d_keep->upload(hits.p, found);
  }
  return found;
}

// --pairs FILE: one pair per non-empty line, "ref_name<TAB>qry_name[<TAB>anything]" -- the names are the file_str of -r / -q
// (a dist TSV can be fed back); with a name that appears twice the first sketch wins.  An unknown name is fatal.
std::vector<hg_ani_hit> read_pair_list(const std::string &path, const Loaded &R, const Loaded &Q) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) die("Opening pair list failed: " + path);
  std::string text;
  char chunk[1 << 16];
  for (size_t got; (got = std::fread(chunk, 1, sizeof chunk, f)) > 0;) text.append(chunk, got);
  std::fclose(f);
  std::map<std::string, uint32_t> by_r, by_q;
  for (size_t i = 0; i < R.n; ++i) by_r.emplace(hg_sketch_file_get(R.f, i)->file_str, (uint32_t)i);  // (emplace keeps the first)
  for (size_t i = 0; i < Q.n; ++i) by_q.emplace(hg_sketch_file_get(Q.f, i)->file_str, (uint32_t)i);
  std::vector<hg_ani_hit> list;
  size_t line_no = 0;
  for (size_t b = 0; b < text.size();) {
    const size_t e = std::min(text.find('\n', b), text.size());
    ++line_no;
    if (e > b) {
      const std::string where = "--pairs " + path + ": line " + std::to_string(line_no) + ": ";
      const size_t t1 = std::min(text.find('\t', b), e);
      if (t1 == e) die(where + "expected ref_name<TAB>qry_name");
      const size_t t2 = std::min(text.find('\t', t1 + 1), e);
      const std::string rn = text.substr(b, t1 - b), qn = text.substr(t1 + 1, t2 - t1 - 1);
      const auto ir = by_r.find(rn);
      if (ir == by_r.end()) die(where + "unknown reference name '" + rn + "'");
      const auto iq = by_q.find(qn);
      if (iq == by_q.end()) die(where + "unknown query name '" + qn + "'");
      list.push_back(hg_ani_hit{ir->second, iq->second, 0.0f});
    }
    b = e + 1;
  }
  if (list.size() > 0xFFFFFFFFull) die("--pairs " + path + ": more than 2^32 - 1 pairs");
  return list;
}

// "<file_str of A's record a>\t<file_str of B's record b>\t<ani>\n" ("{}\t{}\t{:.3}\n", src/utils.rs:277-282) at w: two memcpy and
// put_ani, at most A.len[a] + B.len[b] + 10 bytes
inline size_t put_line(char *w, const Loaded &A, size_t a, const Loaded &B, size_t b, float ani) {
  char *const w0 = w;
  w += A.put_name(w, a);
  *w++ = '\t';
  w += B.put_name(w, b);
  w += put_ani(w, ani);
  return (size_t)(w - w0);
}
inline size_t put_u32(char *o, uint32_t v) {  // decimal, at most 10 digits
  char tmp[10];
  size_t n = 0, k = 0;
  do tmp[n++] = (char)('0' + v % 10), v /= 10;
  while (v);
  while (n) o[k++] = tmp[--n];
  return k;
}

// One TSV file of `items` items: put(i, w) writes item i at w and returns its bytes, at most bound(i) of them.  -t threads
// format contiguous ranges of the items, one part per 4096 items at the most, and every part then goes to its own offset of
// the file: the copies into the page cache run side by side.  Returns the size of the file.
template <class Bound, class Put>
size_t write_tsv(const std::string &path, unsigned threads, size_t items, Bound bound, Put put, const char *failed) {
  double tp = now_s();
  const size_t FT = std::max<size_t>(1, std::min<size_t>(threads, items / 4096 + 1));
  std::vector<std::string> part(FT);
  parallel(FT, [&](size_t t) {
    const size_t lo = items * t / FT, hi = items * (t + 1) / FT;
    size_t need = 0;
    for (size_t i = lo; i < hi; ++i) need += bound(i);
    std::string &o = part[t];
    o.resize(need);
    char *w = &o[0];
    for (size_t i = lo; i < hi; ++i) w += put(i, w);
    o.resize((size_t)(w - &o[0]));
  });
  std::vector<size_t> at(FT + 1, 0);
  for (size_t t = 0; t < FT; ++t) at[t + 1] = at[t] + part[t].size();
  debugf("TSV formatted (%.1f MB) in %.1f ms", at[FT] / 1e6, (now_s() - tp) * 1e3);
  tp = now_s();
  const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
  if (fd < 0) die(failed);
  std::atomic<bool> bad{false};
  parallel(FT, [&](size_t t) {
    const char *p = part[t].data();
    size_t left = part[t].size(), off = at[t];
    while (left) {
      const ssize_t w = ::pwrite(fd, p, left, (off_t)off);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) {
        bad = true;
        return;
      }
      p += w, off += (size_t)w, left -= (size_t)w;
    }
  });
  if (::close(fd) != 0 || bad) die(failed);
  debugf("TSV written in %.1f ms", (now_s() - tp) * 1e3);
  return at[FT];
}

// What dist, search and cluster work on: the devices, one sketch file or two, and their rows on the devices (the caller's
// to_devices fills dR / dQ).  The devices are opened on a thread of their own -- the HIP runtime comes up (~0.2 s) while the
// files are read and parsed, two of them side by side.  (die() leaves through _exit: nothing is torn down on that path.)
struct Session {
  hg_multi *multi = nullptr;
  Loaded R, Q2;  // Q2: the second file, where there is one
  const bool two;
  DevSet dR, dQ;
  Session(unsigned shards, int ani_metric, const std::string &path_r, const std::string *path_q = nullptr) : two(path_q != nullptr) {
    const double tp = now_s();
    std::thread opener([&] {
      multi = open_all_devices(shards);
      ckm(multi, hg_multi_set_ani_metric(multi, ani_metric), "ani_metric");
      debugf("devices opened in %.1f ms", (now_s() - tp) * 1e3);
    });
    std::thread second;
    if (two) second = std::thread([&] { load(*path_q, Q2); });
    load(path_r, R);
    if (two) second.join();
    debugf("sketch files loaded in %.1f ms", (now_s() - tp) * 1e3);
    opener.join();
    if (R.ksize != Q().ksize) die("Ref and query sketches use different kmer sizes!");
    if (R.hv_d != Q().hv_d) die("Ref and query sketches use different HV dimensions!");
  }
  Session(const Session &) = delete;
  ~Session() {
    release(multi, dR), release(multi, dQ);
    hg_sketch_file_free(R.f);
    if (two) hg_sketch_file_free(Q2.f);
    hg_multi_destroy(multi);
  }
  const Loaded &Q() const { return two ? Q2 : R; }  // the query side: the one file against itself without a second
};

// The genomes of a sketch file written with sketch --fragment: consecutive records whose names differ only in a final
// :<digits>-<digits>.  A record without that suffix is a genome of one fragment; a genome whose name reappears behind
// another one is fatal.
struct Genomes {
  std::vector<uint32_t> first;  // n + 1 record offsets
  std::vector<std::string> name;
  size_t n() const { return name.size(); }
};
std::string genome_of(const char *record) {
  const std::string s = record;
  size_t e = s.size(), d = e;
  while (d && std::isdigit((unsigned char)s[d - 1])) --d;
  if (d == e || !d || s[d - 1] != '-') return s;
  size_t b = d - 1;
  while (b && std::isdigit((unsigned char)s[b - 1])) --b;
  if (b == d - 1 || b < 2 || s[b - 1] != ':') return s;  // (a name that is nothing but the suffix stays whole)
  return s.substr(0, b - 1);
}
Genomes genomes_of(const Loaded &L, const std::string &path) {
  Genomes G;
  std::map<std::string, bool> seen;
  for (size_t i = 0; i < L.n; ++i) {
    const char *record = hg_sketch_file_get(L.f, i)->file_str;
    std::string g = genome_of(record);
    if (!G.name.empty() && g == G.name.back()) continue;
    if (!seen.emplace(g, true).second)
      die(path + ": genome '" + g + "' reappears at record '" + record + "' behind another genome: the fragments of a genome must be consecutive");
    G.first.push_back((uint32_t)i), G.name.push_back(std::move(g));
  }
  G.first.push_back((uint32_t)L.n);
  return G;
}

void dump_text(const std::string &path, const std::string &text, const char *failed) {
  FILE *f = std::fopen(path.c_str(), "wb");
  const bool bad = !f || std::fwrite(text.data(), 1, text.size(), f) != text.size();
  if ((f && std::fclose(f) != 0) || bad) die(failed);
}
std::string milli_str(uint64_t v) {  // thousandths with exactly three decimals
  char buf[32];
  std::snprintf(buf, sizeof buf, "%llu.%03llu", (unsigned long long)(v / 1000), (unsigned long long)(v % 1000));
  return buf;
}
uint64_t milli_of(float ani) {  // the integer dist prints for an ANI (put_ani), which is the library's m
  if (!(ani >= 0.0f)) ani = 0.0f;
  if (ani > 100.0f) ani = 100.0f;
  return (uint64_t)__builtin_rint((double)ani * 1000.0);
}

// dist --fragments: the sketches of -r are reference windows, those of -q query fragments; hg_frag_ani_dev reduces the
// (windows x fragments) matrix, block by block on the first visible GPU, to one record per pair of genomes -- and with
// --fragment_hits to every fragment's best window per reference genome.  Everything printed is an integer of thousandths.
int run_dist_fragments(const Cli &c) {
  const double t0 = now_s();
  const bool sym = c.path_r == c.path_q;
  Session s(1, c.ani_metric, c.path_r, sym ? nullptr : &c.path_q);
  const Loaded &R = s.R, &Q = s.Q();
  const Genomes gr = genomes_of(R, c.path_r), gq = sym ? gr : genomes_of(Q, c.path_q);
  to_devices(s.multi, R, s.dR);
  if (!sym) to_devices(s.multi, Q, s.dQ);
  const DevSet &dq = sym ? s.dR : s.dQ;
  logline("INFO", "Computing fragment ANI..");
  hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
  const size_t n_ref = gr.n(), n_qry = gq.n();
  const bool want_hits = given(c, "fragment_hits");
  std::vector<hg_frag_pair> pair(n_ref * n_qry);
  std::vector<hg_frag_best> best(want_hits ? n_ref * Q.n : 0);
  {
    DevBuf<hg_frag_pair> d_pair(ctx, pair.size());
    DevBuf<hg_frag_best> d_best(ctx);
    if (want_hits) d_best.alloc(best.size());
    ck(ctx, hg_frag_ani_dev(ctx, s.dR.hv[0], s.dR.n2[0], R.n, dq.hv[0], dq.n2[0], Q.n, (uint32_t)R.hv_d, R.ksize, gr.first.data(), n_ref,
                            gq.first.data(), n_qry, c.fragment_ani, 0, d_pair.get(), want_hits ? d_best.get() : nullptr), "fragment ANI");
    d_pair.download(pair.data(), pair.size());
    if (want_hits) d_best.download(best.data(), best.size());
  }
  const uint64_t a_milli = milli_of(c.ani_th), m_th = milli_of(c.fragment_ani);
  std::string text;
  size_t lines = 0;
  for (size_t h = 0; h < n_qry; ++h)
    for (size_t g = 0; g < n_ref; ++g) {
      const hg_frag_pair &p = pair[g * n_qry + h];
      if (!p.matched || p.matched < c.min_fragments) continue;
      const uint64_t ani = (2 * p.sum + p.matched) / (2ull * p.matched);
      if (ani < a_milli) continue;
      text += gr.name[g] + "\t" + gq.name[h] + "\t" + milli_str(ani) + "\t" + std::to_string(p.matched) + "\t" + std::to_string(p.total) + "\n";
      ++lines;
    }
  dump_text(c.out, text, "Dump ANI file failed!");
  char buf[512];
  std::snprintf(buf, sizeof buf, "Output %zu of %zu genome pairs with at least %llu fragments at %.1f and ANI above %.1f to file %s", lines,
                n_ref * n_qry, c.min_fragments, c.fragment_ani, c.ani_th, c.out.c_str());
  logline("INFO", buf);
  if (want_hits) {
    text.clear();
    size_t hits = 0;
    for (size_t q = 0; q < Q.n; ++q)
      for (size_t g = 0; g < n_ref; ++g) {
        const hg_frag_best &b = best[g * Q.n + q];
        if (b.row == HG_FRAG_NONE || b.m < m_th) continue;
        text += std::string(hg_sketch_file_get(Q.f, q)->file_str) + "\t" + hg_sketch_file_get(R.f, b.row)->file_str + "\t" + milli_str(b.m) + "\n";
        ++hits;
      }
    dump_text(c.fragment_hits, text, "Dump fragment hits file failed!");
    std::snprintf(buf, sizeof buf, "Output %zu fragment hits to file %s", hits, c.fragment_hits.c_str());
    logline("INFO", buf);
  }
  std::snprintf(buf, sizeof buf, "Computed fragment ANIs for %zu ref genomes (%zu windows) and %zu query genomes (%zu fragments) took %.3fs", n_ref,
                R.n, n_qry, Q.n, now_s() - t0);
  logline("INFO", buf);
  return 0;
}

int run_dist(const Cli &c) {
  if (c.path_r == "1" || c.path_q == "1" || c.out.empty())
    die("the following required arguments were not provided: --path_r --path_q --out");
  if (given(c, "fragments")) return run_dist_fragments(c);
  const double t0 = now_s();
  const bool sym = c.path_r == c.path_q;  // src/dist.rs:13
  // (containment is directional: one file against itself runs the full comparison and writes every ordered pair i != j)
  const bool sym_full = sym && c.ani_metric == HG_ANI_CONTAINMENT;
  // --columns / --pairs: the pairs' further metrics come from one hg_ani_pairs_dev call on the device list, on one GPU
  // --newick: the neighbour-joining tree of the file's sketches (hg_nj_dev), on that GPU too
  // --histogram: the counts of all pairs' ANI values (hg_hist_dev), a second pass on that GPU
  const bool pairs = given(c, "pairs"), newick = given(c, "newick"), with_cols = pairs || given(c, "columns"), histogram = given(c, "histogram");
  const bool one_gpu = with_cols || newick || histogram;
  const uint32_t metric_bit = c.ani_metric == HG_ANI_MASH ? HG_PAIRS_MASH : c.ani_metric == HG_ANI_CONTAINMENT ? HG_PAIRS_CONTAINMENT : HG_PAIRS_MAX_CONTAINMENT;
  uint32_t mask = pairs ? metric_bit : 0u;  // (--pairs: the ANI field itself is a column of the call)
  for (const uint32_t b : c.columns) mask |= b;
  const size_t n_cols = (size_t)__builtin_popcount(mask);
  auto col_at = [&](uint32_t bit) { return (size_t)__builtin_popcount(mask & (bit - 1)); };  // a column's place in a pair's values
  Session s(one_gpu ? 1 : c.shards, c.ani_metric, c.path_r, sym ? nullptr : &c.path_q);
  const Loaded &R = s.R, &Q = s.Q();
  const DevSet &dq = sym ? s.dR : s.dQ;
  double tp = now_s();
  to_devices(s.multi, R, s.dR);
  if (!sym) to_devices(s.multi, Q, s.dQ);
  debugf("payloads uploaded and decompressed on the device(s) in %.1f ms", (now_s() - tp) * 1e3);
  logline("INFO", "Computing ANI..");
  tp = now_s();
  const size_t total = sym_full ? R.n * (R.n - 1) : (sym ? R.n * (Q.n - 1) / 2 : R.n * Q.n);
  HitBuf hits;
  std::vector<float> cols;  // --columns / --pairs: n_cols values per line, in ascending order of the column bits
  size_t found = 0;
  {
    hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
    DevBuf<hg_ani_hit> d_list(ctx);  // ... and the device list they are computed on
    if (pairs) {
      const std::vector<hg_ani_hit> list = read_pair_list(c.pairs_file, R, Q);
      found = list.size();
      hits.resize(found);
      if (found) {
        std::memcpy(hits.p, list.data(), found * sizeof(hg_ani_hit));
        d_list.alloc(found);
        d_list.upload(hits.p, found);
      }
    } else {
      // (ordered on the device: dump_ani_file's order, src/utils.rs:262-269 -- two stable radix passes instead of a comparison
      // sort of up to 10^6..10^8 triples on one host core)
      const bool full = sym_full || !sym;
      found = all_hits(s.multi, R, s.dR, full ? &Q : nullptr, full ? &dq : nullptr, c.ani_th, true, hits, with_cols ? &d_list : nullptr);
    }
    if (with_cols && found) {  // the columns of the ordered device list, before the download
      DevBuf<float> d_cols(ctx, found * n_cols);
      ck(ctx, hg_ani_pairs_dev(ctx, s.dR.hv[0], s.dR.n2[0], R.n, dq.hv[0], dq.n2[0], Q.n, (uint32_t)R.hv_d, R.ksize, d_list.get(), found,
                               mask, d_cols.get(), nullptr), "ani_pairs");
      cols.resize(found * n_cols);
      d_cols.download(cols.data(), cols.size());
      if (pairs) {
        for (size_t i = 0; i < found; ++i) hits.p[i].ani = cols[i * n_cols + col_at(metric_bit)];
      } else {
        hits.resize(found);
        d_list.download(hits.p, found);
      }
    }
  }
  std::vector<hg_nj_join> joins;  // --newick: the tree's joins, computed while the sketches are on the device
  if (newick) {
    hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
    const double tn = now_s();
    DevBuf<hg_nj_join> d_joins(ctx, std::max<size_t>(R.n, 2) - 1);
    size_t n_joins = 0;
    ck(ctx, hg_nj_dev(ctx, s.dR.hv[0], s.dR.n2[0], R.n, (uint32_t)R.hv_d, R.ksize, d_joins.get(), &n_joins), "nj");
    joins.resize(n_joins);
    if (n_joins) d_joins.download(joins.data(), n_joins);
    debugf("neighbour joining of %zu sketches in %.1f ms", R.n, (now_s() - tn) * 1e3);
  }
  std::vector<uint64_t> hist;  // --histogram: the counts, computed while the sketches are on the device
  if (histogram) {
    hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
    const double th = now_s();
    hist.resize(hg_hist_bins(c.histogram_bin));
    DevBuf<uint64_t> d_hist(ctx, hist.size());
    // dist's own enumeration: i != j of the one file under containment, i < j of the one file, everything of two files
    ck(ctx, hg_hist_dev(ctx, s.dR.hv[0], s.dR.n2[0], R.n, dq.hv[0], dq.n2[0], Q.n, (uint32_t)R.hv_d, R.ksize,
                        sym_full ? HG_HIST_OFFDIAG : sym ? HG_HIST_UPPER : HG_HIST_ALL, c.histogram_bin, 0, d_hist.get()), "histogram");
    d_hist.download(hist.data(), hist.size());
    debugf("histogram of all pairs in %zu bins in %.1f ms", hist.size(), (now_s() - th) * 1e3);
  }
  if (sym_full && !pairs) {  // (the pairs i = j are not written: the order of the rest stays)
    size_t w = 0;
    for (size_t i = 0; i < found; ++i)
      if (hits.p[i].ref_idx != hits.p[i].qry_idx) {
        if (n_cols) std::copy_n(cols.begin() + i * n_cols, n_cols, cols.begin() + w * n_cols);
        hits.p[w++] = hits.p[i];
      }
    found = w;
  }
  debugf("ANI matrix (%zu hits), ordered, on the host in %.1f ms", found, (now_s() - tp) * 1e3);
  // one line per hit, in the order of the hits; --columns: one further field each, over the line's '\n'
  write_tsv(c.out, c.threads, found,
            [&](size_t i) { return (size_t)R.len[hits.p[i].ref_idx] + Q.len[hits.p[i].qry_idx] + 10 + 10 * c.columns.size(); },
            [&](size_t i, char *w) {
              const hg_ani_hit &h = hits.p[i];
              size_t k = put_line(w, R, h.ref_idx, Q, h.qry_idx, h.ani);
              for (const uint32_t b : c.columns) --k, k += put_ani(w + k, cols[i * n_cols + col_at(b)]);
              return k;
            },
            "Dump ANI file failed!");
  char buf[512];
  const double perc = total ? 100.0 * found / total : 0.0;
  if (pairs) {
    std::snprintf(buf, sizeof buf, "Output %zu listed ANIs to file %s", found, c.out.c_str());
    logline("INFO", buf);
  } else if (perc < 5.0) {
    std::snprintf(buf, sizeof buf, "Output ANIs with threshold %.1f are too divergent: %zu of %zu (%.2f%%) ANIs are reported",
                  c.ani_th, found, total, perc);
    logline("WARN", buf);
  } else {
    std::snprintf(buf, sizeof buf, "Output %zu of %zu ANIs above threshold %.1f to file %s", found, total, c.ani_th, c.out.c_str());
    logline("INFO", buf);
  }
  if (newick) {
    std::vector<const char *> names(R.n);
    for (size_t i = 0; i < R.n; ++i) names[i] = hg_sketch_file_get(R.f, i)->file_str;
    char *text = nullptr;
    size_t len = 0;
    if (hg_nj_newick(joins.data(), R.n, names.data(), &text, &len) != HG_OK) die("inconsistent neighbour-joining result");
    dump_text(c.newick_out, std::string(text, len), "Dump Newick file failed!");
    hg_free(text);
    std::snprintf(buf, sizeof buf, "Output neighbour-joining tree of %zu genomes to file %s", R.n, c.newick_out.c_str());
    logline("INFO", buf);
  }
  if (histogram) {  // one line per bin: first and last printed value, pairs, pairs in this and all higher bins
    std::vector<uint64_t> above(hist.size() + 1, 0);
    for (size_t b = hist.size(); b-- > 0;) above[b] = above[b + 1] + hist[b];
    std::string text;
    for (size_t b = 0; b < hist.size(); ++b) {
      const uint64_t lo = b * (uint64_t)c.histogram_bin, hi = std::min<uint64_t>(lo + c.histogram_bin - 1, HG_HIST_MILLI_MAX);
      text += milli_str(lo) + "\t" + milli_str(hi) + "\t" + std::to_string(hist[b]) + "\t" + std::to_string(above[b]) + "\n";
    }
    dump_text(c.histogram_out, text, "Dump histogram file failed!");
    std::snprintf(buf, sizeof buf, "Output ANI histogram of %llu pairs in %zu bins of width %s to file %s", (unsigned long long)above[0], hist.size(),
                  milli_str(c.histogram_bin).c_str(), c.histogram_out.c_str());
    logline("INFO", buf);
  }
  std::snprintf(buf, sizeof buf, "Computed ANIs for %zu ref files and %zu query files took %.3fs", R.n, Q.n, now_s() - t0);
  logline("INFO", buf);
  return 0;
}

// `search`: the reference parses the subcommand and does nothing (src/main.rs:22-24, "TODO: support for search").
// Here: every query sketch against the reference database, the top_n (-n, default 1) references per query with
// ANI >= ani_th, one line "query<TAB>reference<TAB>ani" per result, queries in file order, best first.
// Without -r / -q / -o it stays the reference's no-op.
int run_search(const Cli &c) {
  if (c.path_r == "1" || c.path_q == "1" || c.out.empty()) return 0;
  const double t0 = now_s();
  Session s(c.shards, c.ani_metric, c.path_r, &c.path_q);
  const Loaded &R = s.R, &Q = s.Q2;
  double tp = now_s();
  const uint32_t k = std::max(1u, c.top_n);
  // The fused path (hg_search_topk_multi_dev): the k best per query are selected on the device while blocks of the ANI
  // matrix stream past -- no hit list, memory does not depend on how many pairs lie above the threshold.  Every shard keeps
  // its reference rows and holds ALL queries.  -n beyond HG_SEARCH_TOPK_MAX (or --search_path hits) takes the hit list.
  const bool fused = c.search_path == SearchPath::topk || (c.search_path == SearchPath::automatic && k <= HG_SEARCH_TOPK_MAX);
  to_devices(s.multi, R, s.dR);
  to_devices(s.multi, Q, s.dQ, fused);
  debugf("payloads uploaded and decompressed on the device(s) in %.1f ms", (now_s() - tp) * 1e3);
  logline("INFO", "Searching..");
  tp = now_s();
  std::vector<hg_ani_hit> best(Q.n * (size_t)k);
  std::vector<uint32_t> cnt(Q.n);
  if (fused) {
    ckm(s.multi, hg_search_topk_multi_dev(s.multi, s.dR.hv.data(), s.dR.n2.data(), s.dR.rows.data(), s.dQ.hv.data(), s.dQ.n2.data(), Q.n,
                                          (uint32_t)R.hv_d, R.ksize, c.ani_th, k, best.data(), cnt.data()), "search");
    debugf("top-%u per query, selected block by block, in %.1f ms", k, (now_s() - tp) * 1e3);
  } else {
    HitBuf hits;
    hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
    DevBuf<hg_ani_hit> d_hits(ctx);
    const size_t found = all_hits(s.multi, R, s.dR, &Q, &s.dQ, c.ani_th, false, hits, &d_hits);
    debugf("ANI matrix (%zu hits) in %.1f ms", found, (now_s() - tp) * 1e3);
    tp = now_s();
    DevBuf<hg_ani_hit> d_out(ctx, best.size());
    DevBuf<uint32_t> d_cnt(ctx, cnt.size());
    ck(ctx, hg_topk_per_query_dev(ctx, d_hits.get(), found, Q.n, k, d_out.get(), d_cnt.get()), "top-k");
    d_out.download(best.data(), best.size());
    d_cnt.download(cnt.data(), cnt.size());
    debugf("top-%u per query in %.1f ms", k, (now_s() - tp) * 1e3);
  }
  tp = now_s();
  std::vector<size_t> at;  // the place in `best` of every result to report: queries in file order, best first
  for (size_t q = 0; q < Q.n; ++q)
    for (size_t r = 0; r < std::min<uint32_t>(cnt[q], k); ++r) at.push_back(q * k + r);
  const size_t tsv_bytes = write_tsv(c.out, c.threads, at.size(),
                                     [&](size_t i) { return (size_t)Q.len[at[i] / k] + R.len[best[at[i]].ref_idx] + 10; },
                                     [&](size_t i, char *w) { return put_line(w, Q, at[i] / k, R, best[at[i]].ref_idx, best[at[i]].ani); },
                                     "Dump search file failed!");
  debugf("TSV formatted and written (%.1f MB) in %.1f ms", tsv_bytes / 1e6, (now_s() - tp) * 1e3);
  char buf[256];
  std::snprintf(buf, sizeof buf, "Searched %zu queries against %zu references: %zu results (top %u, ANI >= %.1f) took %.3fs",
                Q.n, R.n, at.size(), k, c.ani_th, now_s() - t0);
  logline("INFO", buf);
  return 0;
}

// `cluster` (an extension: the reference has no such subcommand): single-linkage clusters of the sketches of one file at an
// ANI threshold, computed where the hits are (hg_cluster_dev: the symmetric comparison in row blocks, each block's hits
// unioned on the device).  One line per sketch record, in file order: "<file_str>\t<cluster id>\t<file_str of the
// cluster's first member>\n" -- ids count the clusters in the order of their first members.
// --linkage greedy (hg_cluster_greedy_dev): one representative per cluster, the sketches processed in file order or
// (--order size) by descending hv_norm_2, ties in file order.  The rows go to the library in processing order -- the decode
// offsets of the upload are permuted, nothing is gathered on the device -- and the lines stay in file order:
// "<file_str>\t<cluster id>\t<file_str of its representative>\t<ANI with it, as dist prints it>\n"; ids count the
// representatives in processing order.
// --linkage setcover (hg_cluster_setcover_dev): greedy set cover -- the sketch with the most still-uncovered neighbours
// becomes a representative and takes them as its members.  The lines are those of greedy, in file order; a representative
// may stand behind its members in the file.
// --hclust average, --agglomerate average (hg_cluster_average_dev): average linkage on the dense matrix.  The lines of
// single linkage; --tree writes the merges, every child before its parent: "<file_str of the name that stays>\t<file_str
// of the absorbed name>\t<average ANI of the merge, as dist prints it>\t<size of the merged cluster>\n".
// --agglomerate complete (hg_cluster_complete_dev): complete linkage on the dense matrix.  The same lines; the third field
// of a --tree line is the lowest ANI between the two merged clusters.
// --stats <file> (hg_cluster_stats_dev): one line per cluster at -a, whatever formed the clusters -- the statistics of the
// device arrays as they stand, in processing order under --order size, so that ties go to the sketch processed first.
//
// What a scheme leaves on the host: the clusters at -a, in processing order, and what only some schemes produce
struct Cut {  // the clusters at one threshold
  float th;
  size_t n_cl = 0;
  std::vector<uint32_t> rep, cl;
};
struct Merge {  // the absorbed name, what it went into, the merge's level and size
  uint32_t name, into, size;
  float level;
};
struct Clusters {
  Cut at;                              // -a
  std::vector<float> ani;              // greedy, setcover: every sketch's ANI with its representative
  std::vector<Merge> merges;           // average, complete with --tree: the dendrogram, every child before its parent
  std::vector<hg_ani_hit> tree;        // --tree / --levels: the edges of the single-linkage tree
  std::vector<Cut> more;               // --levels: one further threshold each, cut from the tree
  std::vector<hg_cluster_stat> stats;  // --stats
};

// A scheme's device calls: the sketches as they lie on the device, the arrays the clusters at -a go to, and one function per
// scheme that fills what it produces of `r` beyond them (r.at.rep and r.at.cl are downloaded by the caller)
struct ClusterJob {
  const Cli &c;
  const Loaded &L;
  hg_ctx *ctx;
  const int16_t *hv;
  const int32_t *n2;
  uint32_t *d_rep, *d_cl;
  const float th = c.ani_th;

  // --hclust average, --agglomerate: the schemes on the dense matrix
  void dense(Clusters &r) const {
    const bool want = given(c, "tree");
    DevBuf<uint32_t> d_into(ctx), d_size(ctx);  // (NULL without --tree: the library then skips the dendrogram)
    DevBuf<float> d_level(ctx);
    if (want) d_into.alloc(L.n), d_size.alloc(L.n), d_level.alloc(L.n);
    ck(ctx, (c.complete ? hg_cluster_complete_dev : hg_cluster_average_dev)(ctx, hv, n2, L.n, (uint32_t)L.hv_d, L.ksize, th, d_rep, d_cl,
                                                                            d_into.get(), d_level.get(), d_size.get(), &r.at.n_cl),
       "cluster");
    if (c.complete) debugf("complete linkage in %llu rounds", (unsigned long long)hg_ctx_cluster_complete_rounds(ctx));
    else debugf("average linkage in %llu rounds", (unsigned long long)hg_ctx_cluster_average_rounds(ctx));
    if (!want) return;
    std::vector<uint32_t> into(L.n), sz(L.n);
    std::vector<float> level(L.n);
    d_into.download(into.data(), L.n), d_size.download(sz.data(), L.n), d_level.download(level.data(), L.n);
    for (size_t i = 0; i < L.n; ++i)
      if (into[i] != i) r.merges.push_back(Merge{(uint32_t)i, into[i], sz[i], level[i]});
    // averages, and minima, never increase towards the root: by (level descending, size ascending, into, name) children come first
    std::sort(r.merges.begin(), r.merges.end(), [](const Merge &x, const Merge &y) {
      if (x.level != y.level) return x.level > y.level;
      if (x.size != y.size) return x.size < y.size;
      if (x.into != y.into) return x.into < y.into;
      return x.name < y.name;
    });
  }
  // --linkage greedy | setcover: one representative per cluster
  void representatives(Clusters &r) const {
    const bool setcover = c.linkage == Linkage::setcover;
    DevBuf<float> d_ani(ctx, L.n);
    ck(ctx, (setcover ? hg_cluster_setcover_dev : hg_cluster_greedy_dev)(ctx, hv, n2, L.n, (uint32_t)L.hv_d, L.ksize, th, d_rep, d_cl,
                                                                         d_ani.get(), &r.at.n_cl), "cluster");
    r.ani.resize(L.n);
    d_ani.download(r.ani.data(), L.n);
    if (setcover) debugf("set-cover resolution in %llu rounds", (unsigned long long)hg_ctx_cluster_setcover_rounds(ctx));
    else debugf("greedy resolution in %llu rounds", (unsigned long long)hg_ctx_cluster_greedy_rounds(ctx));
  }
  // --tree, --levels: one comparison at the floor -a (hg_cluster_tree_dev); every level is a cut of the tree (the step calls of
  // hg_cluster)
  void tree_and_levels(Clusters &r) const {
    DevBuf<hg_ani_hit> d_tree(ctx, std::max<size_t>(L.n, 2));
    size_t n_edges = 0;
    ck(ctx, hg_cluster_tree_dev(ctx, hv, n2, L.n, (uint32_t)L.hv_d, L.ksize, th, d_tree.get(), L.n ? L.n - 1 : 0, &n_edges, d_rep, d_cl,
                                &r.at.n_cl), "cluster");
    debugf("tree of %zu edges in %llu rounds", n_edges, (unsigned long long)hg_ctx_cluster_tree_rounds(ctx));
    r.tree.resize(n_edges);
    if (n_edges) d_tree.download(r.tree.data(), n_edges);
    DevBuf<uint32_t> d_rep2(ctx, L.n), d_cl2(ctx, L.n);  // (one pair of buffers for all levels)
    for (const float t : c.levels) {
      Cut v;
      v.th = t, v.rep.resize(L.n), v.cl.resize(L.n);
      ck(ctx, hg_cluster_init_dev(ctx, d_rep2.get(), L.n), "cluster");
      ck(ctx, hg_cluster_add_hits_dev(ctx, d_rep2.get(), L.n, d_tree.get(), n_edges, t), "cluster");
      ck(ctx, hg_cluster_finish_dev(ctx, d_rep2.get(), L.n, d_cl2.get(), &v.n_cl), "cluster");
      d_rep2.download(v.rep.data(), L.n);
      d_cl2.download(v.cl.data(), L.n);
      r.more.push_back(std::move(v));
    }
  }
  void single(Clusters &r) const {
    ck(ctx, hg_cluster_dev(ctx, hv, n2, L.n, (uint32_t)L.hv_d, L.ksize, th, d_rep, d_cl, &r.at.n_cl), "cluster");
  }
  // --stats: the records of the clusters at -a, from the device arrays as they stand (processing order)
  void stats(Clusters &r) const {
    const double ts = now_s();
    const size_t n_cl = r.at.n_cl;
    DevBuf<hg_cluster_stat> d_stat(ctx, std::max<size_t>(n_cl, 1));
    ck(ctx, hg_cluster_stats_dev(ctx, hv, n2, L.n, (uint32_t)L.hv_d, L.ksize, d_cl, n_cl, nullptr, d_stat.get()), "cluster statistics");
    r.stats.resize(n_cl);
    if (n_cl) d_stat.download(r.stats.data(), n_cl);
    debugf("cluster statistics in %.1f ms", (now_s() - ts) * 1e3);
  }
};

// Everything the writers index with, before anything is written
void check_clusters(const Cli &c, size_t n, const Clusters &r) {
  const bool setcover = c.linkage == Linkage::setcover;
  bool bad = (c.hclust_average || c.complete) && given(c, "tree") && r.merges.size() != n - r.at.n_cl;
  for (const Merge &m : r.merges) bad |= m.into > m.name;
  // (a set-cover representative may have a larger index than its member)
  for (size_t i = 0; i < n; ++i) bad |= r.at.cl[i] >= r.at.n_cl || (setcover ? r.at.rep[i] >= n : r.at.rep[i] > i);
  for (const Cut &v : r.more)
    for (size_t i = 0; i < n; ++i) bad |= v.cl[i] >= v.n_cl || v.rep[i] > i;
  if (given(c, "tree"))
    for (const hg_ani_hit &e : r.tree) bad |= e.ref_idx >= n || e.qry_idx >= n;
  for (const hg_cluster_stat &x : r.stats)
    bad |= x.size == 0 || x.medoid >= n || (x.size >= 2 && (x.within_min_a >= n || x.within_min_b >= n)) ||
           (x.outside_idx != HG_STATS_NONE && (x.outside_member >= n || x.outside_idx >= n));
  if (bad) die("inconsistent cluster result");
}

// "Output N genomes in M clusters (S singletons) at ANI threshold <th> to file <-o>"
void log_cut(const Cli &c, size_t n, const Cut &v, const char *th) {
  std::vector<uint32_t> size(v.n_cl, 0);
  for (size_t i = 0; i < n; ++i) ++size[v.cl[i]];
  size_t singletons = 0;
  for (uint32_t x : size) singletons += x == 1;
  char buf[512];
  std::snprintf(buf, sizeof buf, "Output %zu genomes in %zu clusters (%zu singletons) at ANI threshold %s to file %s", n, v.n_cl, singletons, th,
                c.out.c_str());
  logline("INFO", buf);
}

// -o: one line per record, in file order: its name, "\t<cluster id>\t<name of the cluster's first member or representative>" for -a
// and for each level, then the ANI with the representative where there are representatives.  perm: processing position -> record
void write_clusters(const Cli &c, const Loaded &L, const std::vector<uint32_t> &perm, const Clusters &r) {
  const std::vector<uint32_t> &rep = r.at.rep, &cl = r.at.cl;
  const std::vector<Cut> &more = r.more;
  std::vector<uint32_t> pos(L.n);  // record -> processing position
  for (size_t k = 0; k < L.n; ++k) pos[perm[k]] = (uint32_t)k;
  write_tsv(c.out, c.threads, L.n,
            [&](size_t i) {
              size_t b = (size_t)L.len[i] + 12 + L.len[perm[rep[pos[i]]]] + 9;
              for (const Cut &v : more) b += 12 + L.len[v.rep[i]];
              return b;
            },
            [&](size_t i, char *w) {
              auto put_cluster = [&](char *o, uint32_t id, size_t first) {
                size_t b = 0;
                o[b++] = '\t', b += put_u32(o + b, id), o[b++] = '\t';
                return b + L.put_name(o + b, first);
              };
              const uint32_t k = pos[i];
              size_t b = L.put_name(w, i);
              b += put_cluster(w + b, cl[k], perm[rep[k]]);
              for (const Cut &v : more) b += put_cluster(w + b, v.cl[i], v.rep[i]);
              if (c.linkage != Linkage::single) return b + put_ani(w + b, r.ani[k]);  // "\t<ani>\n"
              w[b++] = '\n';
              return b;
            },
            "Dump cluster file failed!");
}
// --tree of average and complete linkage: one line per merge: file of into, file of the absorbed name, level, size
void write_merge_tree(const Cli &c, const Loaded &L, const std::vector<Merge> &merges) {
  write_tsv(c.tree_out, c.threads, merges.size(), [&](size_t i) { return (size_t)L.len[merges[i].into] + L.len[merges[i].name] + 22; },
            [&](size_t i, char *w) {
              size_t b = put_line(w, L, merges[i].into, L, merges[i].name, merges[i].level);
              w[b - 1] = '\t';  // (put_line ends the line behind the ANI)
              b += put_u32(w + b, merges[i].size);
              w[b++] = '\n';
              return b;
            },
            "Dump tree file failed!");
}
// --tree of single linkage: one line per edge, strongest first: file of lo, file of hi, ANI as dist prints it
void write_edge_tree(const Cli &c, const Loaded &L, const std::vector<hg_ani_hit> &tree) {
  write_tsv(c.tree_out, c.threads, tree.size(), [&](size_t i) { return (size_t)L.len[tree[i].ref_idx] + L.len[tree[i].qry_idx] + 10; },
            [&](size_t i, char *w) { return put_line(w, L, tree[i].ref_idx, L, tree[i].qry_idx, tree[i].ani); }, "Dump tree file failed!");
}
// --stats: one line per cluster, in id order: id, size, medoid, mean and minimum within (and the pair that has it), the nearest
// sketch outside (its ANI, the member, the sketch, the sketch's cluster); NA where a cluster has no such value
void write_stats(const Cli &c, const Loaded &L, const std::vector<uint32_t> &perm, const Clusters &r) {
  const std::vector<hg_cluster_stat> &stats = r.stats;
  const uint32_t none = HG_STATS_NONE;
  size_t mixed = 0;  // clusters of two or more whose nearest outside sketch is as close as their two least similar members
  for (const hg_cluster_stat &x : stats) mixed += x.size >= 2 && x.outside_idx != none && x.outside_max >= x.within_min;
  auto name_len = [&](uint32_t k) { return k == none ? (size_t)2 : (size_t)L.len[perm[k]]; };
  write_tsv(c.stats_out, c.threads, stats.size(),
            [&](size_t i) {
              const hg_cluster_stat &x = stats[i];
              return 80 + name_len(x.medoid) + name_len(x.within_min_a) + name_len(x.within_min_b) + name_len(x.outside_member) +
                     name_len(x.outside_idx);
            },
            [&](size_t i, char *w) {
              const hg_cluster_stat &x = stats[i];
              size_t b = 0;
              auto tab = [&] { w[b++] = '\t'; };
              auto na = [&] { tab(), w[b++] = 'N', w[b++] = 'A'; };
              auto name = [&](uint32_t k) { tab(), b += L.put_name(w + b, perm[k]); };
              auto milli = [&](uint32_t m) {  // the thousandths as dist prints an ANI
                tab(), b += put_u32(w + b, m / 1000), w[b++] = '.';
                w[b++] = (char)('0' + m / 100 % 10), w[b++] = (char)('0' + m / 10 % 10), w[b++] = (char)('0' + m % 10);
              };
              b += put_u32(w + b, (uint32_t)i), tab(), b += put_u32(w + b, x.size), name(x.medoid);
              if (x.size >= 2) {
                const float mean = (float)(((double)x.within_sum / ((double)x.size * (double)(x.size - 1))) / 1000.0);
                b += put_ani(w + b, mean) - 1;  // (without put_ani's end of line)
                milli(x.within_min), name(x.within_min_a), name(x.within_min_b);
              } else {
                na(), na(), na(), na();
              }
              if (x.outside_idx != none) {
                milli(x.outside_max), name(x.outside_member), name(x.outside_idx);
                tab(), b += put_u32(w + b, r.at.cl[x.outside_idx]);
              } else {
                na(), na(), na(), na();
              }
              w[b++] = '\n';
              return b;
            },
            "Dump statistics file failed!");
  char buf[512];
  std::snprintf(buf, sizeof buf, "Output statistics of %zu clusters (%zu not separated) to file %s", stats.size(), mixed, c.stats_out.c_str());
  logline("INFO", buf);
}

int run_cluster(const Cli &c) {
  if (c.path == "1" || c.out.empty()) die("the following required arguments were not provided: --path --out");
  const double t0 = now_s();
  Session s(1, c.ani_metric, c.path);
  const Loaded &L = s.R;
  std::vector<uint32_t> perm(L.n);  // processing position -> record: the file order unless --order size (greedy only)
  for (size_t i = 0; i < L.n; ++i) perm[i] = (uint32_t)i;
  if (c.order_size) std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return L.n2[a] > L.n2[b]; });
  to_devices(s.multi, L, s.dR, false, c.order_size ? &perm : nullptr);
  char buf[512];
  std::snprintf(buf, sizeof buf, "Clustering %zu genomes at ANI threshold %.1f..", L.n, c.ani_th);
  logline("INFO", buf);
  const double tp = now_s();
  hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
  DevBuf<uint32_t> d_rep(ctx, L.n), d_cl(ctx, L.n);
  const ClusterJob job{c, L, ctx, s.dR.hv[0], s.dR.n2[0], d_rep.get(), d_cl.get()};
  const bool dense = c.hclust_average || c.complete;  // average or complete linkage
  Clusters r;
  r.at.th = c.ani_th, r.at.rep.resize(L.n), r.at.cl.resize(L.n);
  if (dense) job.dense(r);
  else if (c.linkage != Linkage::single) job.representatives(r);
  else if (given(c, "tree") || given(c, "levels")) job.tree_and_levels(r);
  else job.single(r);
  d_rep.download(r.at.rep.data(), L.n);
  d_cl.download(r.at.cl.data(), L.n);
  debugf("clusters on the host in %.1f ms", (now_s() - tp) * 1e3);
  if (given(c, "stats")) job.stats(r);
  check_clusters(c, L.n, r);

  write_clusters(c, L, perm, r);
  if (given(c, "tree")) dense ? write_merge_tree(c, L, r.merges) : write_edge_tree(c, L, r.tree);
  std::snprintf(buf, sizeof buf, "%.1f", r.at.th);
  log_cut(c, L.n, r.at, buf);
  if (given(c, "stats")) write_stats(c, L, perm, r);
  for (const Cut &v : r.more) {
    // (one decimal like -a's line where that is the level, else as many digits as it needs)
    std::snprintf(buf, sizeof buf, "%.1f", (double)v.th);
    if (std::strtof(buf, nullptr) != v.th) std::snprintf(buf, sizeof buf, "%g", (double)v.th);
    log_cut(c, L.n, v, buf);
  }
  std::snprintf(buf, sizeof buf, "Clustered %zu files took %.3fs", L.n, now_s() - t0);
  logline("INFO", buf);
  return 0;
}

// triangle: the ANI of all pairs of one file as fixed-width text (hypergen_tri.h).  Every byte of the file has a closed-form
// place -- "n\n", then per row the name, a separator and the row's fields -- so a block that hg_tri_stream_dev hands over goes
// straight to its rows' offsets, its rows dealt to -t threads, while the device computes and formats the next block.
struct TriangleFile {
  const Loaded &L;
  int fd;
  uint32_t layout;
  unsigned threads;
  size_t head;                   // bytes of the first line
  std::vector<uint64_t> name_at;  // bytes of the names and their separators in front of row i
  std::atomic<bool> bad{false};
  bool write_all(const char *p, size_t left, uint64_t off) {
    while (left) {
      const ssize_t w = ::pwrite(fd, p, left, (off_t)off);
      if (w < 0 && errno == EINTR) continue;
      if (w <= 0) return false;
      p += w, off += (size_t)w, left -= (size_t)w;
    }
    return true;
  }
  // row i: its name, '\t' (a row without fields: '\n') and `bytes` of fields
  bool write_row(size_t i, const char *fields, size_t bytes) {
    std::string name(L.len[i] + 1, bytes ? '\t' : '\n');
    L.put_name(&name[0], i);
    const uint64_t off = head + name_at[i] + hg_tri_field_offset(layout, 0, i, 0, L.n);
    struct iovec iov[2] = {{&name[0], name.size()}, {const_cast<char *>(fields), bytes}};
    ssize_t w;
    do w = ::pwritev(fd, iov, bytes ? 2 : 1, (off_t)off);
    while (w < 0 && errno == EINTR);
    if (w < 0) return false;
    if ((size_t)w == name.size() + bytes) return true;
    // a short write: the rest piece by piece
    const size_t done = (size_t)w;
    if (done < name.size() && !write_all(name.data() + done, name.size() - done, off + done)) return false;
    const size_t of_fields = done > name.size() ? done - name.size() : 0;
    return write_all(fields + of_fields, bytes - of_fields, off + name.size() + of_fields);
  }
  static int sink(void *user, const char *text, size_t, size_t row0, size_t rows) {
    TriangleFile &f = *static_cast<TriangleFile *>(user);
    const size_t T = std::max<size_t>(1, std::min<size_t>(f.threads, rows));
    parallel(T, [&](size_t t) {
      for (size_t i = row0 + rows * t / T, hi = row0 + rows * (t + 1) / T; i < hi && !f.bad; ++i)
        if (!f.write_row(i, text + hg_tri_field_offset(f.layout, row0, i, 0, f.L.n), (size_t)hg_tri_text_bytes(f.layout, i, 1, f.L.n))) f.bad = true;
    });
    return f.bad ? 1 : 0;
  }
};

int run_triangle(const Cli &c) {
  if (c.path == "1" || c.out.empty()) die("the following required arguments were not provided: --path --out");
  const double t0 = now_s();
  const uint32_t layout = c.ani_metric == HG_ANI_CONTAINMENT ? HG_TRI_FULL : HG_TRI_LOWER;  // (the directional metric: every ordered pair)
  Session s(1, c.ani_metric, c.path);
  const Loaded &L = s.R;
  to_devices(s.multi, L, s.dR);
  logline("INFO", "Computing ANI..");
  const double tp = now_s();
  hg_ctx *ctx = hg_multi_ctx(s.multi, 0);
  const char *const failed = "Dump matrix file failed!";
  const int fd = ::open(c.out.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
  if (fd < 0) die(failed);
  const std::string first = std::to_string(L.n) + "\n";
  TriangleFile f{L, fd, layout, c.threads ? c.threads : 1u, first.size(), std::vector<uint64_t>(L.n + 1, 0)};
  for (size_t i = 0; i < L.n; ++i) f.name_at[i + 1] = f.name_at[i] + L.len[i] + 1;
  if (!f.write_all(first.data(), first.size(), 0)) die(failed);
  const hg_status st = hg_tri_stream_dev(ctx, s.dR.hv[0], s.dR.n2[0], L.n, (uint32_t)L.hv_d, L.ksize, layout, 0, TriangleFile::sink, &f);
  if (f.bad || st == HG_ERR_IO) die(failed);
  ck(ctx, st, "triangle");
  if (::close(fd) != 0) die(failed);
  const uint64_t size = f.head + f.name_at[L.n] + hg_tri_text_bytes(layout, 0, L.n, L.n);
  debugf("matrix of %.1f MB computed, formatted and written in %.1f ms", size / 1e6, (now_s() - tp) * 1e3);
  char buf[512];
  std::snprintf(buf, sizeof buf, "Output ANI matrix of %zu sketches (%s) to file %s", L.n, layout == HG_TRI_LOWER ? "lower triangle" : "square", c.out.c_str());
  logline("INFO", buf);
  std::snprintf(buf, sizeof buf, "Computed ANI matrix of %zu files took %.3fs", L.n, now_s() - t0);
  logline("INFO", buf);
  return 0;
}
}  // namespace

int main(int argc, char **argv) {
  const Cli c = parse(argc, argv);
  // (a normal return: leaving through _exit once the outputs are closed saves the runtime's exit handlers -- 20-40 ms of a
  // 10 000 x 10 000 dist -- but those handlers are also where rocprofv3 and other tools write what they collected)
  if (c.mode_bit == SKETCH) return run_sketch(c);
  if (c.mode_bit == DIST) return run_dist(c);
  if (c.mode_bit == CLUSTER) return run_cluster(c);
  if (c.mode_bit == TRIANGLE) return run_triangle(c);
  return run_search(c);
}
