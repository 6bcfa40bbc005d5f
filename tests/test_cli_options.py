"""The option surface of the command line, argument vector by argument vector: the exit status and the exact stderr of
`hyper-gen` for every option in every form it has, every kind of bad value, every subcommand that refuses an option and
every rule between options on both sides of its edge.  Option faults are reported before any file or device is opened,
so nothing here needs a GPU and nothing may create a file.  The expected outcomes are literals on purpose: they were
recorded from the hand-written option switch that the option table replaced, and the table has to reproduce them."""
import os
import re
import subprocess

import pytest

import hypergen_amd as hg


# (arguments, exit status, stderr)
CASES = [
    # every option in every form it has (search without -r / -q / -o is a no-op: exit 0, nothing printed)
    (('search', '--path', 'a', '--path_r', 'b', '--path_q', 'c', '--thread', '4', '--sketch_method', 'm', '--canonical', 'false', '--ksize', '31', '--seed', '7', '--scaled', '100', '--hv_d', '1024', '--quant_scale', '2.0', '--ani_th', '90', '--device', 'gpu', '--top_n', '3', '--pack_layout', 'naive', '--ani_metric', 'containment', '--shards', '2', '--search_path', 'hits'), 0, ''),
    (('search', '--path=a', '--path_r=b', '--path_q=c', '--thread=4', '--sketch_method=m', '--canonical=false', '--ksize=31', '--seed=7', '--scaled=100', '--hv_d=1024', '--quant_scale=2.0', '--ani_th=90', '--device=gpu', '--top_n=3', '--pack_layout=naive', '--ani_metric=containment', '--shards=2', '--search_path=hits'), 0, ''),
    (('search', '-p', 'a', '-r', 'b', '-q', 'c', '-t', '4', '-m', 'm', '-C', 'false', '-k', '31', '-S', '7', '-s', '100', '-d', '1024', '-Q', '2.0', '-a', '90', '-D', 'gpu', '-n', '3', '-L', 'naive', '-G', '2'), 0, ''),
    (('search', '-pa', '-rb', '-qc', '-t4', '-mm', '-Cfalse', '-k31', '-S7', '-s100', '-d1024', '-Q2.0', '-a90', '-Dgpu', '-n3', '-Lnaive', '-G2'), 0, ''),
    (('search', '-p=a', '-r=b', '-q=c', '-t=4', '-m=m', '-C=false', '-k=31', '-S=7', '-s=100', '-d=1024', '-Q=2.0', '-a=90', '-D=gpu', '-n=3', '-L=naive', '-G=2'), 0, ''),
    (('search', '-o', 'out.tsv', '--out', 'out.tsv', '--out=out.tsv', '-oout.tsv', '-o=out.tsv'), 0, ''),
    (('search', '-r', 'a', '-q', 'b'), 0, ''),
    (('search', '--pack_layout', 'bitpacker8x', '-L', 'avx2', '-C', 'true', '--ani_metric=mash', '--ani_metric', 'max_containment'), 0, ''),
    (('search', '-a', 'abc', '-Q', 'x'), 0, ''),
    (('cluster', '--linkage', 'greedy', '--order', 'size'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--linkage=setcover'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--linkage=greedy', '--order=file'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--tree', 't.tsv', '--levels', '96,97'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--tree=t.tsv', '--levels=96,97', '-a', '95.5'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--ani_metric', 'max_containment'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('dist', '--columns', 'containment_ref,mash', '--pairs', 'f'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '--columns=mash,containment,max_containment,containment_ref', '--pairs=f'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('sketch', '--min_count', '2'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--min_count=4294967295', '--shards', '2'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    # a choice out of a fixed list, with a value that is not in it
    (('search', '--canonical', 'maybe'), 2, "error: invalid value 'maybe' for '--canonical'\n"),
    (('search', '-C', 'yes'), 2, "error: invalid value 'yes' for '--canonical'\n"),
    (('search', '--ani_metric', 'jaccard'), 2, "error: invalid value 'jaccard' for '--ani_metric' (mash | containment | max_containment)\n"),
    (('search', '--search_path', 'fast'), 2, "error: invalid value 'fast' for '--search_path' (auto | hits | topk)\n"),
    (('cluster', '--linkage', 'complete'), 2, "error: invalid value 'complete' for '--linkage' (single | greedy | setcover)\n"),
    (('dist', '--linkage', 'cover'), 2, "error: invalid value 'cover' for '--linkage' (single | greedy | setcover)\n"),
    (('cluster', '--order', 'big'), 2, "error: invalid value 'big' for '--order' (file | size)\n"),
    (('sketch', '--pack_layout', 'sse'), 2, "error: invalid value 'sse' for '--pack_layout' (avx2 | naive)\n"),
    (('sketch', '-L=foo'), 2, "error: invalid value 'foo' for '--pack_layout' (avx2 | naive)\n"),
    (('search', '--canonical='), 2, "error: invalid value '' for '--canonical'\n"),
    # numbers: empty, not a number, negative, over the range, and the last value inside it
    (('search', '-t', ''), 2, "error: invalid value '' for '-t'\n"),
    (('search', '-t', 'abc'), 2, "error: invalid value 'abc' for '-t'\n"),
    (('search', '-t', '-1'), 2, "error: invalid value '-1' for '-t'\n"),
    (('search', '-t', '256'), 2, "error: invalid value '256' for '-t'\n"),
    (('search', '-t', '255'), 0, ''),
    (('search', '--thread=256'), 2, "error: invalid value '256' for '--thread=256'\n"),
    (('search', '-t256'), 2, "error: invalid value '256' for '-t256'\n"),
    (('search', '-t=256'), 2, "error: invalid value '256' for '-t=256'\n"),
    (('search', '--thread', '4x'), 2, "error: invalid value '4x' for '--thread'\n"),
    (('search', '-k', ''), 2, "error: invalid value '' for '-k'\n"),
    (('search', '-k', 'x'), 2, "error: invalid value 'x' for '-k'\n"),
    (('search', '-k', '-1'), 2, "error: invalid value '-1' for '-k'\n"),
    (('search', '-k', '256'), 2, "error: invalid value '256' for '-k'\n"),
    (('search', '-k', '255'), 0, ''),
    (('search', '-S', ''), 2, "error: invalid value '' for '-S'\n"),
    (('search', '-S', 'x'), 2, "error: invalid value 'x' for '-S'\n"),
    (('search', '-S', '-1'), 0, ''),
    (('search', '-S', '18446744073709551616'), 0, ''),
    (('search', '-s', ''), 2, "error: invalid value '' for '-s'\n"),
    (('search', '-s', '1e3'), 2, "error: invalid value '1e3' for '-s'\n"),
    (('search', '-d', ''), 2, "error: invalid value '' for '-d'\n"),
    (('search', '--hv_d', '0x10'), 2, "error: invalid value '0x10' for '--hv_d'\n"),
    (('search', '-n', ''), 2, "error: invalid value '' for '-n'\n"),
    (('search', '-n', 'x'), 2, "error: invalid value 'x' for '-n'\n"),
    (('search', '-n', '-1'), 2, "error: invalid value '-1' for '-n'\n"),
    (('search', '-n', '1048577'), 2, "error: invalid value '1048577' for '-n'\n"),
    (('search', '-n', '1048576'), 0, ''),
    (('search', '--shards', ''), 2, "error: invalid value '' for '--shards'\n"),
    (('search', '--shards', 'x'), 2, "error: invalid value 'x' for '--shards'\n"),
    (('search', '--shards', '-1'), 2, "error: invalid value '-1' for '--shards'\n"),
    (('search', '--shards', '65'), 2, "error: invalid value '65' for '--shards'\n"),
    (('search', '--shards', '64'), 0, ''),
    (('search', '-G', '65'), 2, "error: invalid value '65' for '-G'\n"),
    (('sketch', '--min_count', ''), 2, "error: invalid value '' for '--min_count'\n"),
    (('sketch', '--min_count', 'x'), 2, "error: invalid value 'x' for '--min_count'\n"),
    (('sketch', '--min_count', '-1'), 2, "error: invalid value '-1' for '--min_count'\n"),
    (('sketch', '--min_count', '0'), 2, "error: invalid value '0' for '--min_count'\n"),
    (('sketch', '--min_count=0'), 2, "error: invalid value '0' for '--min_count=0'\n"),
    (('sketch', '--min_count', '4294967296'), 2, "error: invalid value '4294967296' for '--min_count'\n"),
    # a value is missing, an option or a word is unknown
    (('search', '-t'), 2, "error: a value is required for '-t'\n"),
    (('search', '--thread'), 2, "error: a value is required for '--thread'\n"),
    (('search', '--levels'), 2, "error: a value is required for '--levels'\n"),
    (('search', '-x'), 2, "error: a value is required for '-x'\n"),
    (('search', '--thread='), 2, "error: invalid value '' for '--thread='\n"),
    (('search', '--bogus', '1'), 2, "error: unexpected argument '--bogus'\n"),
    (('search', '--bogus=1'), 2, "error: unexpected argument '--bogus=1'\n"),
    (('search', '--bogus'), 2, "error: unexpected argument '--bogus'\n"),
    (('search', '-x', '1'), 2, "error: unexpected argument '-x'\n"),
    (('search', '-x1'), 2, "error: unexpected argument '-x1'\n"),
    (('search', 'word'), 2, "error: unexpected argument 'word'\n"),
    (('search', '-'), 2, "error: unexpected argument '-'\n"),
    (('search', '--'), 2, "error: unexpected argument '--'\n"),
    (('search', '-t', '4', 'word'), 2, "error: unexpected argument 'word'\n"),
    (('search', '-t', '300', '--bogus'), 2, "error: invalid value '300' for '-t'\n"),
    (('frobnicate',), 2, "error: unknown subcommand 'frobnicate'\n"),
    ((), 2, 'error: usage: hyper-gen <sketch|dist|search|cluster> [options]   (see --help)\n'),
    # an option in a subcommand that refuses it
    (('sketch', '--search_path', 'hits'), 2, 'error: --search_path is not supported by sketch: it chooses how search selects its results\n'),
    (('dist', '--search_path', 'hits'), 2, 'error: --search_path is not supported by dist: it chooses how search selects its results\n'),
    (('cluster', '--search_path', 'hits'), 2, 'error: --search_path is not supported by cluster: it chooses how search selects its results\n'),
    (('sketch', '--linkage', 'greedy'), 2, 'error: --linkage is not supported by sketch: it chooses how cluster forms its clusters\n'),
    (('dist', '--linkage', 'greedy'), 2, 'error: --linkage is not supported by dist: it chooses how cluster forms its clusters\n'),
    (('search', '--linkage', 'greedy'), 2, 'error: --linkage is not supported by search: it chooses how cluster forms its clusters\n'),
    (('sketch', '--tree', 't.tsv'), 2, 'error: --tree is not supported by sketch: it belongs to cluster --linkage single\n'),
    (('dist', '--tree', 't.tsv'), 2, 'error: --tree is not supported by dist: it belongs to cluster --linkage single\n'),
    (('search', '--tree', 't.tsv'), 2, 'error: --tree is not supported by search: it belongs to cluster --linkage single\n'),
    (('sketch', '--levels', '97'), 2, 'error: --levels is not supported by sketch: it belongs to cluster --linkage single\n'),
    (('dist', '--levels', '97'), 2, 'error: --levels is not supported by dist: it belongs to cluster --linkage single\n'),
    (('search', '--levels', '97'), 2, 'error: --levels is not supported by search: it belongs to cluster --linkage single\n'),
    (('sketch', '--columns', 'mash'), 2, "error: --columns is not supported by sketch: it adds a pair's other metrics to the lines of dist\n"),
    (('search', '--columns', 'mash'), 2, "error: --columns is not supported by search: it adds a pair's other metrics to the lines of dist\n"),
    (('cluster', '--columns', 'mash'), 2, "error: --columns is not supported by cluster: it adds a pair's other metrics to the lines of dist\n"),
    (('sketch', '--pairs', 'f'), 2, 'error: --pairs is not supported by sketch: it names the pairs dist evaluates\n'),
    (('search', '--pairs', 'f'), 2, 'error: --pairs is not supported by search: it names the pairs dist evaluates\n'),
    (('cluster', '--pairs', 'f'), 2, 'error: --pairs is not supported by cluster: it names the pairs dist evaluates\n'),
    (('dist', '--min_count', '2'), 2, 'error: --min_count is not supported by dist: the filter needs the k-mer counts, which a sketch no longer has\n'),
    (('search', '--min_count', '2'), 2, 'error: --min_count is not supported by search: the filter needs the k-mer counts, which a sketch no longer has\n'),
    (('cluster', '--min_count', '2'), 2, 'error: --min_count is not supported by cluster: the filter needs the k-mer counts, which a sketch no longer has\n'),
    (('cluster', '--shards', '2', '-p', 'x', '-o', 'out.tsv'), 2, 'error: --shards is not supported by cluster: it runs on the first visible GPU\n'),
    (('cluster', '-G', '2', '-p', 'x', '-o', 'out.tsv'), 2, 'error: --shards is not supported by cluster: it runs on the first visible GPU\n'),
    (('cluster', '--ani_metric', 'containment', '-p', 'x', '-o', 'out.tsv'), 2, 'error: --ani_metric containment is not supported by cluster: it is directional (mash | max_containment)\n'),
    (('cluster', '--shards', '0'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('dist', '--search_path', 'hits', '--linkage', 'greedy'), 2, 'error: --search_path is not supported by dist: it chooses how search selects its results\n'),
    (('sketch', '--tree', 't.tsv', '--levels', '97'), 2, 'error: --tree is not supported by sketch: it belongs to cluster --linkage single\n'),
    (('cluster', '--columns', 'mash', '--pairs', 'f', '--min_count', '2'), 2, "error: --columns is not supported by cluster: it adds a pair's other metrics to the lines of dist\n"),
    # an option that does not go with --shards
    (('cluster', '--tree', 't.tsv', '--shards', '2'), 2, 'error: --tree is not supported with --shards: cluster runs on the first visible GPU\n'),
    (('cluster', '--shards', '2', '--levels', '97'), 2, 'error: --levels is not supported with --shards: cluster runs on the first visible GPU\n'),
    (('dist', '--columns', 'mash', '--shards', '2'), 2, 'error: --columns is not supported with --shards: dist with --columns or --pairs runs on the first visible GPU\n'),
    (('dist', '--shards=2', '--pairs', 'f'), 2, 'error: --pairs is not supported with --shards: dist with --columns or --pairs runs on the first visible GPU\n'),
    (('dist', '--columns', 'mash', '--shards', '0'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    # what an option needs of the others, on both sides of the edge
    (('cluster', '--order', 'size'), 2, 'error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n'),
    (('cluster', '--linkage', 'single', '--order', 'file'), 2, 'error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n'),
    (('cluster', '--linkage', 'setcover', '--order', 'file'), 2, "error: --order is not supported by cluster --linkage setcover: the order the representatives are chosen in is the rule's own\n"),
    (('dist', '--order', 'size'), 2, 'error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n'),
    (('search', '--order', 'file'), 2, 'error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n'),
    (('cluster', '--linkage', 'greedy', '--tree', 't.tsv'), 2, 'error: --tree needs cluster --linkage single: greedy clusters are not nested and have no tree\n'),
    (('cluster', '--linkage', 'setcover', '--tree', 't.tsv'), 2, 'error: --tree needs cluster --linkage single: set-cover clusters are not nested and have no tree\n'),
    (('cluster', '--linkage', 'single', '--tree', 't.tsv'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--linkage', 'greedy', '--levels', '97'), 2, 'error: --levels needs cluster --linkage single: greedy clusters are not nested and have no tree\n'),
    (('cluster', '--linkage', 'setcover', '--levels', '97'), 2, 'error: --levels needs cluster --linkage single: set-cover clusters are not nested and have no tree\n'),
    (('cluster', '--levels', '95'), 2, "error: invalid value for '--levels': every level must be above -a, the threshold the tree is built at\n"),
    (('cluster', '--levels', '95.1'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '-a', '97', '--levels', '97'), 2, "error: invalid value for '--levels': every level must be above -a, the threshold the tree is built at\n"),
    (('cluster', '-a', '97', '--levels', '97.5'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '--levels', '98,99', '-a', '98'), 2, "error: invalid value for '--levels': every level must be above -a, the threshold the tree is built at\n"),
    (('search', '--search_path', 'topk', '-n', '64'), 0, ''),
    (('search', '--search_path', 'topk', '-n', '65'), 2, 'error: --search_path topk takes -n up to 64 (larger -n goes through the hit list)\n'),
    (('search', '-n65', '--search_path=topk'), 2, 'error: --search_path topk takes -n up to 64 (larger -n goes through the hit list)\n'),
    (('search', '-n', '65', '--search_path', 'hits'), 0, ''),
    (('search', '-n', '65', '--search_path', 'auto'), 0, ''),
    # the comma lists
    (('cluster', '--levels', ''), 2, "error: invalid value '' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels', '97,,99'), 2, "error: invalid value '97,,99' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels=97,,99'), 2, "error: invalid value '97,,99' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels', '97,'), 2, "error: invalid value '97,' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels', 'abc'), 2, "error: invalid value 'abc' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels', 'nan'), 2, "error: invalid value 'nan' for '--levels' (1 to 8 ANI thresholds, comma-separated, ascending)\n"),
    (('cluster', '--levels', '99,97'), 2, "error: invalid value '99,97' for '--levels': the levels must be strictly ascending\n"),
    (('cluster', '--levels', '97,97'), 2, "error: invalid value '97,97' for '--levels': the levels must be strictly ascending\n"),
    (('cluster', '--levels', '96,96.5,97,97.5,98,98.5,99,99.5,99.9'), 2, "error: invalid value '96,96.5,97,97.5,98,98.5,99,99.5,99.9' for '--levels': at most 8 levels\n"),
    (('cluster', '--levels', '96,96.5,97,97.5,98,98.5,99,99.5'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('dist', '--columns', 'nonsense'), 2, "error: invalid value 'nonsense' for '--columns' (a comma list out of mash, containment, containment_ref, max_containment)\n"),
    (('dist', '--columns', 'mash,mash'), 2, "error: invalid value 'mash,mash' for '--columns': 'mash' is listed twice\n"),
    (('dist', '--columns', 'mash,,containment'), 2, "error: invalid value 'mash,,containment' for '--columns' (a comma list out of mash, containment, containment_ref, max_containment)\n"),
    (('dist', '--columns', ''), 2, "error: invalid value '' for '--columns' (a comma list out of mash, containment, containment_ref, max_containment)\n"),
    (('dist', '--columns', ','), 2, "error: invalid value ',' for '--columns' (a comma list out of mash, containment, containment_ref, max_containment)\n"),
    (('dist', '--columns', 'mash,Containment'), 2, "error: invalid value 'mash,Containment' for '--columns' (a comma list out of mash, containment, containment_ref, max_containment)\n"),
    (('cluster', '--tree', ''), 2, "error: invalid value '' for '--tree' (a file name)\n"),
    (('dist', '--pairs='), 2, "error: invalid value '' for '--pairs' (a file name)\n"),
    # required arguments
    (('sketch',), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '-p', 'x'), 2, 'error: the following required arguments were not provided: --out\n'),
    (('dist',), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '-r', 'a', '-q', 'b'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '-o', 'out.tsv'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('cluster',), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '-p', 'x'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('cluster', '-o', 'out.tsv'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('search',), 0, ''),
    # the ten options that parse once read by hand (--alphabet, --translate, --individual, --min_length, --fragment,
    # --fragment_step, --fragments, --fragment_ani, --min_fragments, --fragment_hits), recorded from those readers before they
    # became rows of the table: a bad number is reported under the option's bare name however it was typed, a switch takes no
    # '=value', and the first fault reported is the one of the earlier row
    (('sketch', '--individual', '--min_length=x'), 2, "error: invalid value 'x' for '--min_length'\n"),
    (('sketch', '--fragment=x'), 2, "error: invalid value 'x' for '--fragment'\n"),
    (('sketch', '--fragment', '8', '--fragment_step=x'), 2, "error: invalid value 'x' for '--fragment_step'\n"),
    (('dist', '--fragments', '--min_fragments=0'), 2, "error: invalid value '0' for '--min_fragments'\n"),
    (('dist', '--fragments', '--fragment_ani=101'), 2, "error: invalid value '101' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (('dist', '--fragments', '--fragment_hits='), 2, "error: invalid value '' for '--fragment_hits' (a file name)\n"),
    (('sketch', '--alphabet='), 2, "error: invalid value '' for '--alphabet' (dna | protein)\n"),
    (('sketch', '--alphabet', 'rna'), 2, "error: invalid value 'rna' for '--alphabet' (dna | protein)\n"),
    (('sketch', '--alphabet'), 2, "error: a value is required for '--alphabet'\n"),
    (('sketch', '--translate=1'), 2, "error: unexpected argument '--translate=1'\n"),
    (('sketch', '--min_length', '--individual'), 2, "error: invalid value '--individual' for '--min_length'\n"),
    (('dist', '--alphabet', 'protein', '--search_path', 'hits'), 2, 'error: --search_path is not supported by dist: it chooses how search selects its results\n'),
    (('dist', '--translate', '--individual'), 2, 'error: --translate is not supported by dist: it translates the nucleotide sequences sketch reads\n'),
    (('search', '--fragment_ani', '95', '--fragment', '8'), 2, 'error: --fragment is not supported by search: it cuts the sequences sketch reads into windows\n'),
    (('cluster', '--min_length', '5', '--alphabet', 'dna'), 2, 'error: --alphabet is not supported by cluster: it names the alphabet of the sequences sketch reads\n'),
    (('search', '--fragments', '--tree', 't'), 2, 'error: --tree is not supported by search: it belongs to cluster --linkage single\n'),
    (('dist', '--fragment_hits', 'h', '--min_fragments', '2'), 2, 'error: --min_fragments needs --fragments: without it dist compares whole sketches\n'),
    (('dist', '--fragment_ani', '95', '--search_path', 'topk', '-n', '65'), 2, 'error: --search_path is not supported by dist: it chooses how search selects its results\n'),
    (('dist', '--fragments', '--fragment_ani', '95', '--shards', '2', '--columns', 'mash'), 2, 'error: --columns is not supported with --shards: dist with --columns or --pairs runs on the first visible GPU\n'),
    (('sketch', '--fragments', '--min_count', '0'), 2, "error: invalid value '0' for '--min_count'\n"),
    (('sketch', '--fragment', '8', '-t', '300'), 2, "error: invalid value '300' for '-t'\n"),
    (('sketch', '-t', '300', '--fragment', 'x'), 2, "error: invalid value '300' for '-t'\n"),
    (('sketch', '--individual', '--fragment_step', '8'), 2, 'error: --fragment_step needs --fragment: without it sketch makes one sketch per file\n'),
    (('sketch', '--alphabet', 'protein', '--alphabet', 'dna', '--fragment', '1000'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--translate', '--translate'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    # ... their values: missing, empty, out of range, the last one inside it
    (('sketch', '--individual=1'), 2, "error: unexpected argument '--individual=1'\n"),
    (('dist', '--fragments='), 2, "error: unexpected argument '--fragments='\n"),
    (('sketch', '--translate', 'x'), 2, "error: unexpected argument 'x'\n"),
    (('sketch', '--min_length'), 2, "error: a value is required for '--min_length'\n"),
    (('sketch', '--min_length='), 2, "error: invalid value '' for '--min_length'\n"),
    (('sketch', '--individual', '--min_length', '-1'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--fragment=8x'), 2, "error: invalid value '8x' for '--fragment'\n"),
    (('sketch', '--fragment_step'), 2, "error: a value is required for '--fragment_step'\n"),
    (('sketch', '--fragment', '18446744073709551616'), 2, "error: invalid value '18446744073709551615' for '--fragment': a window is a multiple of 4 bases, at least 4\n"),
    (('dist', '--fragments', '--min_fragments=4294967296'), 2, "error: invalid value '4294967296' for '--min_fragments'\n"),
    (('dist', '--fragments', '--min_fragments', '4294967295'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '--fragments', '--fragment_ani=nan'), 2, "error: invalid value 'nan' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (('dist', '--fragments', '--fragment_ani', '-1'), 2, "error: invalid value '-1' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (('dist', '--fragments', '--fragment_ani', '1e2'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '--fragments', '--fragment_ani='), 2, "error: invalid value '' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (('dist', '--fragments', '--fragment_ani', '95x'), 2, "error: invalid value '95x' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (('dist', '--fragment_ani'), 2, "error: a value is required for '--fragment_ani'\n"),
    # ... in a subcommand that refuses them
    (('search', '--individual'), 2, 'error: --individual is not supported by search: it splits the FASTA files sketch reads into their records\n'),
    (('cluster', '--fragments'), 2, 'error: --fragments is not supported by cluster: it makes dist compare genomes fragment by fragment\n'),
    (('cluster', '--translate'), 2, 'error: --translate is not supported by cluster: it translates the nucleotide sequences sketch reads\n'),
    (('dist', '--fragment_step', '4'), 2, 'error: --fragment_step is not supported by dist: it cuts the sequences sketch reads into windows\n'),
    (('dist', '--fragment', '8', '--fragment_step', '4'), 2, 'error: --fragment is not supported by dist: it cuts the sequences sketch reads into windows\n'),
    (('search', '--min_fragments', '2', '--fragment_hits', 'h'), 2, 'error: --min_fragments is not supported by search: it belongs to dist --fragments\n'),
    # ... and what they need of the others, on both sides of the edge
    (('dist', '--fragment_hits=h'), 2, 'error: --fragment_hits needs --fragments: without it dist compares whole sketches\n'),
    (('dist', '--fragment_ani', '95'), 2, 'error: --fragment_ani needs --fragments: without it dist compares whole sketches\n'),
    (('dist', '--fragments', '--fragment_ani', '95', '--min_fragments', '2', '--fragment_hits', 'h'), 2, 'error: the following required arguments were not provided: --path_r --path_q --out\n'),
    (('dist', '--fragments', '--pairs', 'f'), 2, 'error: --pairs is not supported with --fragments: every pair of genomes is compared\n'),
    (('dist', '--fragments', '--columns', 'mash'), 2, 'error: --columns is not supported with --fragments: a line carries the fragment ANI, the matched and the total fragments\n'),
    (('dist', '--fragments', '--newick', 't'), 2, 'error: --newick is not supported with --fragments: the tree is drawn from whole sketches\n'),
    (('dist', '--fragments', '--shards', '2'), 2, 'error: --shards is not supported with --fragments: it runs on the first visible GPU\n'),
    (('sketch', '--translate', '--alphabet', 'protein'), 2, 'error: --translate is not supported with --alphabet protein: protein input is not translated\n'),
    (('sketch', '--individual', '--alphabet', 'protein'), 2, 'error: --individual is not supported with --alphabet protein: protein input is sketched one file at a time\n'),
    (('sketch', '--individual', '--translate'), 2, 'error: --individual is not supported with --translate: translated input is sketched one file at a time\n'),
    (('sketch', '--individual', '--shards', '2'), 2, 'error: --shards is not supported with --individual: the records are sketched on the first visible GPU\n'),
    (('sketch', '--min_length', '5'), 2, 'error: --min_length needs --individual: without it sketch makes one sketch per file, whatever its length\n'),
    (('sketch', '--individual', '--min_length', '5'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--individual', '--min_length=5'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--translate', '--min_count', '2'), 2, 'error: --min_count is not supported with --translate: amino-acid k-mers are sketched without the count filter\n'),
    (('sketch', '--translate', '--shards', '2'), 2, 'error: --shards is not supported with --translate: translated input is sketched on the first visible GPU\n'),
    (('sketch', '--alphabet', 'protein', '-k', '33'), 2, "error: invalid value '33' for '--ksize': --alphabet protein takes k-mers of 1 to 32 residues\n"),
    (('sketch', '--translate', '-k', '33'), 2, "error: invalid value '33' for '--ksize': --translate takes k-mers of 1 to 32 residues\n"),
    (('sketch', '--alphabet=protein', '-k', '32'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--fragment', '6'), 2, "error: invalid value '6' for '--fragment': a window is a multiple of 4 bases, at least 4\n"),
    (('sketch', '--fragment', '0'), 2, "error: invalid value '0' for '--fragment': a window is a multiple of 4 bases, at least 4\n"),
    (('sketch', '--fragment', '8', '--fragment_step', '12'), 2, "error: invalid value '12' for '--fragment_step': a step above the window would leave bases out\n"),
    (('sketch', '--fragment', '8', '--fragment_step', '6'), 2, "error: invalid value '6' for '--fragment_step': a step is a multiple of 4 bases, at least 4\n"),
    (('sketch', '--fragment', '8', '--fragment_step', '0'), 2, "error: invalid value '0' for '--fragment_step': a step is a multiple of 4 bases, at least 4\n"),
    (('sketch', '--fragment', '8'), 2, "error: invalid value '8' for '--fragment': a window shorter than -k holds no k-mer\n"),
    (('sketch', '--fragment', '24', '--fragment_step=8'), 2, 'error: the following required arguments were not provided: --path --out\n'),
    (('sketch', '--fragment', '8', '--individual'), 2, "error: --fragment is not supported with --individual: the windows are cut from a file's merged sequence, not from its records\n"),
    (('sketch', '--fragment', '8', '--alphabet', 'protein'), 2, 'error: --fragment is not supported with --alphabet protein: protein input is sketched one file at a time\n'),
    (('sketch', '--fragment', '8', '--translate'), 2, 'error: --fragment is not supported with --translate: translated input is sketched one file at a time\n'),
    (('sketch', '--fragment', '8', '--shards', '2'), 2, 'error: --shards is not supported with --fragment: the windows are sketched on the first visible GPU\n'),
    # search has no help of its own: the lookup by subcommand leaves --help and -h to the table, as the three blocks did
    (('search', '--help'), 2, "error: unexpected argument '--help'\n"),
    (('search', '-h'), 2, "error: a value is required for '-h'\n"),
    (('search', '-h', 'x'), 2, "error: unexpected argument '-h'\n"),
]

HELP = (
    'HyperGen: Fast and memory-efficient genome sketching in hyperdimensional space (MI355X build)\n'
    '\n'
    '  hyper-gen sketch -p {fna_path} -o {output_sketch_file}\n'
    '  hyper-gen dist -r {ref_sketch} -q {query_sketch} -o {output_ANI_results}\n'
    '  hyper-gen search -r {ref_sketch} -q {query_sketch} -o {top_hits_per_query} [-n top_n]\n'
    '  hyper-gen cluster -p {sketch_file} -o {output_clusters} [-a 95.0] [--linkage single|greedy|setcover]\n'
    '                    [--tree {output_tree}] [--levels L1,L2,...]\n'
    '\n'
    'options: -p --path, -r --path_r, -q --path_q, -o --out, -t --thread [16], -m --sketch_method,\n'
    '         -C --canonical [true], -k --ksize [21], -S --seed [123], -s --scaled [1500], -d --hv_d [4096],\n'
    '         -Q --quant_scale [1.0], -a --ani_th [85.0], -D --device [cpu]\n'
    'extensions: -n --top_n [1] (search), --pack_layout avx2|naive [avx2] (sketch: the payload layout of\n'
    '         reference hosts with / without AVX2; dist and search read both), --shards N (dist / search: N\n'
    '         shards dealt round the visible GPUs; default one per GPU), cluster (single-linkage clusters at\n'
    '         -a --ani_th [95.0] on the first visible GPU: one line per sketch, file, cluster id, file of the\n'
    "         cluster's first member), --ani_metric mash|containment|max_containment [mash] (dist / search /\n"
    "         cluster: containment = the share of the query's hashes found in the reference -- the identity of a\n"
    '         fragment, a partial MAG or a draft with a larger genome; max_containment = the same against the\n'
    '         smaller of the two; dist on one file with containment writes every ordered pair i != j; cluster\n'
    '         takes mash or max_containment), --min_count N [1] (sketch: keep a sampled k-mer only if it occurs\n'
    '         at least N times in the file -- for raw reads, where every sequencing error makes k-mers that occur\n'
    "         once; 1 = every sampled k-mer, the reference's set), --search_path auto|hits|topk [auto] (search:\n"
    '         topk selects the -n best per query on the device while blocks of the ANI matrix stream past -- memory\n'
    '         does not grow with the number of pairs above -a; hits builds the thresholded hit list first; auto =\n'
    '         topk for -n <= 64, hits beyond; both write the same file), --linkage single|greedy|setcover [single]\n'
    '         (cluster: greedy = one representative per cluster, as dereplication tools choose them -- a sketch is\n'
    '         a representative unless an earlier representative is within -a of it, else it joins the best such\n'
    '         one; representatives are pairwise below -a, every member is within -a of its own; one line per\n'
    '         sketch: file, cluster id, file of its representative, ANI with it -- 100 for a representative;\n'
    '         setcover = greedy set cover, as MMseqs2 and Linclust cluster: the sketch with the most still-uncovered\n'
    '         neighbours within -a becomes a representative and takes them as its members, ties to the first in\n'
    '         the file, until none is left -- the guarantees and the lines of greedy, the representative chosen by\n'
    '         coverage instead of file order; it holds the hits of the whole comparison, 12 bytes per pair within -a),\n'
    '         --order file|size [file] (cluster --linkage greedy: the order the sketches are processed in; size =\n'
    '         descending hv_norm_2, ties in file order -- the most complete genome of a group represents it;\n'
    '         cluster ids count the representatives in that order, the lines stay in file order),\n'
    '         --tree <file> (cluster --linkage single: the single-linkage tree at the floor -a -- the maximum-ANI\n'
    '         spanning forest, genomes - clusters lines, strongest first: file, file, ANI as dist prints it; cut\n'
    "         at any threshold >= -a it gives that threshold's clusters, its order is the merge order),\n"
    '         --levels L1,L2,... (cluster --linkage single: 1 to 8 further thresholds, ascending, above -a, all from\n'
    '         one comparison at -a; every line of -o becomes file, then for -a and each level the cluster id and\n'
    "         the file of the cluster's first member),\n"
    '         --columns LIST (dist: a comma list out of mash, containment, containment_ref, max_containment; every\n'
    "         line gets one further field per name, in the order listed -- the pair's ANI under that metric, whatever\n"
    "         --ani_metric selected the lines; containment_ref = the share of the reference's hashes found in the\n"
    '         query; runs on the first visible GPU),\n'
    '         --pairs FILE (dist: evaluate the pairs FILE lists, ref_name<TAB>qry_name[<TAB>anything] per line, names\n'
    '         as -r and -q carry them -- a dist TSV can be fed back; one line per listed pair in the order of the\n'
    '         list, ANI under --ani_metric, then the --columns fields; -a is not applied; runs on the first\n'
    '         visible GPU)\n'
)
VERSION = 'hyper-gen 0.0.1 (hypergen-hip 0.1.0 (gfx950))\n'


def run(args, cwd):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, cwd=str(cwd), timeout=60)


@pytest.mark.parametrize("args,code,err", CASES, ids=[" ".join(a) or "(no arguments)" for a, _, _ in CASES])
def test_exit_status_and_stderr(tmp_path, args, code, err):
    r = run(args, tmp_path)
    assert (r.returncode, r.stderr, r.stdout) == (code, err, "")
    assert os.listdir(str(tmp_path)) == []  # neither out.tsv nor t.tsv: the fault, or the no-op, comes before any output


def test_the_matrix_names_every_option_of_the_help_text():
    """a new option has to enter the matrix"""
    named = set(re.findall(r"--[a-z_]+", HELP)) - {"--help", "--version"}
    used = {a.split("=")[0] for args, _, _ in CASES for a in args if a.startswith("--")}
    assert named <= used, sorted(named - used)


@pytest.mark.parametrize("flag", ["--help", "-h"])
def test_help_text_in_full(tmp_path, flag):
    r = run([flag], tmp_path)
    assert (r.returncode, r.stderr) == (0, "") and r.stdout == HELP


@pytest.mark.parametrize("flag", ["--version", "-V"])
def test_version_text_in_full(tmp_path, flag):
    r = run([flag], tmp_path)
    assert (r.returncode, r.stderr) == (0, "") and r.stdout == VERSION
