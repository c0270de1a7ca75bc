"""`scHPF prep | prep-like | train | train-pool | score | project | qc`: command-line entry points over
the loaders, run_trials and the model methods -- argument plumbing only, no logic of its own.

Same sub-commands, options, defaults and output file names as the reference's script
(/root/reference/bin/scHPF:40-292 options; :317-366 prep / prep-like, :370-470 train, :485-534 score,
:536-559 project),
so a pipeline that calls `scHPF train -i X.mtx -o out -k 7 -t 5` keeps working and finds
`out/scHPF_K7_b0_5trials.joblib` (the reference appends `_b{batchsize}` whenever ncells > batchsize,
hence also for batchsize 0).
"""
import argparse
import json
import os
import sys
import time
from functools import partial

import joblib
import numpy as np


def _add_train_options(train, nargs_k=None):
    train.add_argument("-i", "--input", required=True,
                       help="Training data: the .mtx written by `prep`, or a tab-separated "
                            "CELL_ID GENE_ID UMI_COUNT file (0-indexed, no duplicates).")
    train.add_argument("-o", "--outdir", help="Output directory (created if missing).")
    train.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    if nargs_k:
        train.add_argument("-k", "--nfactors", nargs="+", type=int, required=True, help="Numbers of factors.")
    else:
        train.add_argument("-k", "--nfactors", type=int, required=True, help="Number of factors.")
    train.add_argument("-t", "--ntrials", type=int, default=1, help="Random restarts; the best loss wins. [1]")
    train.add_argument("-v", "--validation-cells", default=None,
                       help="Held-out cells (same format as --input) used for convergence and model choice.")
    train.add_argument("-M", "--max-iter", type=int, default=1000, help="Maximum iterations. [1000]")
    train.add_argument("-m", "--min-iter", type=int, default=30, help="Minimum iterations. [30]")
    train.add_argument("-e", "--epsilon", type=float, default=0.001,
                       help="Minimum percent decrease of the loss between checks to continue. [0.001]")
    train.add_argument("-f", "--check-freq", type=int, default=10, help="Iterations between checks. [10]")
    train.add_argument("--better-than-n-ago", default=5, type=int,
                       help="Stop when the loss is worse than this many checks ago and rising. [5]")
    train.add_argument("-a", type=float, default=0.3, help="Hyperparameter a (-2: 1/sqrt(nfactors)). [0.3]")
    train.add_argument("-c", type=float, default=0.3, help="Hyperparameter c (-2: 1/sqrt(nfactors)). [0.3]")
    train.add_argument("--float32", action="store_true", help="32-bit variational parameters.")
    train.add_argument("-bs", "--batchsize", default=0, type=int, help="Cells per training round (0: all).")
    train.add_argument("-sl", "--smooth-loss", default=1, type=int, help="Average the loss over this many checks.")
    train.add_argument("-bts", "--beta-theta-simultaneous", action="store_true",
                       help="Update beta and theta from the previous round's values.")
    train.add_argument("-sa", "--save-all", action="store_true", help="Save every trial.")
    train.add_argument("-rp", "--reproject", action="store_true",
                       help="Reproject the data onto the fixed gene parameters before model selection.")
    train.add_argument("--quiet", dest="verbose", action="store_false", default=True,
                       help="Do not print intermediate losses.")
    train.add_argument("--thin", type=float, default=None, metavar="FRAC",
                       help="Split every count into train and test counts (test ~ Binomial(count, FRAC)), fit on the "
                            "train counts, check convergence and choose the model by the held-out loss on the test "
                            "counts; writes thin_train.mtx and thin_test.mtx beside the model (this build's addition).")
    train.add_argument("--thin-seed", type=int, default=0, metavar="N", help="Seed of the --thin split. [0]")
    train.add_argument("--devices", type=int, nargs="+", default=None,
                       help="HIP device ordinals to spread the restarts over (this build's addition).")


def _parser():
    parser = argparse.ArgumentParser(prog="scHPF", description="scHPF on MI355X")
    sub = parser.add_subparsers(dest="cmd")

    text_or_loom = ("a whitespace-delimited genes x cells UMI count matrix with two leading columns of gene "
                    "attributes (ENSEMBL id, gene name), or a loom file with the row attribute `Accession` or `Gene`")
    prep = sub.add_parser("prep", help="Filter genes and write the training matrix.")
    prep.add_argument("-i", "--input", required=True, help="Input data: " + text_or_loom + ".")
    prep.add_argument("-o", "--outdir", help="Output directory (created if missing; default: the input's).")
    prep.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    prep.add_argument("-m", "--min-cells", type=float, default=0.01,
                      help="Keep genes observed in at least this many cells; a value in (0, 1) is a proportion "
                           "of the cells. [0.01]")
    prep.add_argument("-w", "--whitelist", default="",
                      help="Two-column file (ENSEMBL id, gene name): keep only these genes.")
    prep.add_argument("-b", "--blacklist", default="",
                      help="Two-column file (ENSEMBL id, gene name): drop these genes, also when whitelisted.")
    prep.add_argument("-nvc", "--n-validation-cells", type=int, default=0,
                      help="Hold out this many randomly selected cells for validation. [0]")
    prep.add_argument("-vgid", "--validation-group-ids", default=None,
                      help="Single-column file of cell group ids (np.loadtxt): validation cells are spread "
                           "about evenly over the groups.")
    prep.add_argument("--validation-max-group-frac", type=float, default=0.5,
                      help="With -vgid: the largest share of a group that may be held out. [0.5]")
    prep.add_argument("--filter-by-gene-name", default=False, action="store_true",
                      help="Match the white/blacklist by gene name instead of ENSEMBL id.")
    prep.add_argument("--no-split-on-dot", default=False, action="store_true",
                      help="Accepted for compatibility: the reference ignores it for `prep` (identifiers are "
                           "always compared without their '.version' suffix), and so does this command.")

    like = sub.add_parser("prep-like", help="Write a data set with the genes of another, in the same order.")
    like.add_argument("-i", "--input", required=True, help="Input data: " + text_or_loom + ".")
    like.add_argument("-r", "--reference", required=True,
                      help="Two-column file (ENSEMBL id, gene name), e.g. prep's genes.txt: the genes to select "
                           "from the input, in this order; all must be present.")
    like.add_argument("-o", "--outdir", required=True, help="Output directory (created if missing).")
    like.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    like.add_argument("--by-gene-name", default=False, action="store_true",
                      help="Match against the reference by gene name instead of ENSEMBL id.")
    like.add_argument("--no-split-on-dot", default=False, action="store_true",
                      help="Compare identifiers with their '.version' suffix.")

    train = sub.add_parser("train", help="Train a model (restarts run one after the other on one GPU, or "
                                         "spread over --devices).")
    _add_train_options(train)

    pool = sub.add_parser("train-pool", help="Train several numbers of factors / restarts concurrently.")
    _add_train_options(pool, nargs_k="+")
    pool.add_argument("--njobs", type=int, default=0, help="Concurrent trials (0: as many as devices).")

    score = sub.add_parser("score", help="Write cell scores, gene scores and ranked gene lists as text.")
    score.add_argument("-m", "--model", required=True, help="A .joblib model written by `train`.")
    score.add_argument("-o", "--outdir", default=None,
                       help="Output directory (default: a directory named after the model file).")
    score.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    score.add_argument("-g", "--genefile", default=None,
                       help="Tab-delimited gene table without header (prep's genes.txt): also write ranked genes.")
    score.add_argument("-i", "--input", default=None,
                       help="The count matrix the model was fitted to (same formats as `train -i`): also write the mean "
                            "negative log-likelihood of each cell and each gene (cell_loss.txt, gene_loss.txt).")
    score.add_argument("--ppc", default=False, action="store_true",
                       help="With -i: also write the posterior predictive check per gene and per cell (gene_ppc.txt, "
                            "cell_ppc.txt): predicted mean, variance and fraction of zeros over all entries of the row, "
                            "then the observed ones.")
    score.add_argument("--knn", type=int, default=None, metavar="K",
                       help="Also write the K nearest cells of every cell in factor space, none its own neighbour "
                            "(knn_indices.txt, knn_distances.txt: one row per cell, nearest first).  Needs no count matrix.")
    score.add_argument("--knn-metric", default="euclidean", choices=["euclidean", "cosine"],
                       help="Distance of --knn between cell scores. [euclidean]")
    score.add_argument("--knn-graph", default=None, choices=["umap", "jaccard"],
                       help="With --knn: also write the weighted symmetric graph of the neighbour lists as "
                            "knn_connectivities.mtx: UMAP's fuzzy simplicial set (scanpy's connectivities) or the "
                            "shared-neighbour Jaccard graph.")
    score.add_argument("--clusters", default=False, action="store_true",
                       help="With --knn-graph: also write the Louvain clusters of that graph as clusters.txt, one label "
                            "per cell.")
    score.add_argument("--resolution", type=float, default=None, metavar="R",
                       help="Resolution of --clusters: larger values give more, smaller clusters. [1.0]")
    score.add_argument("--connected", default=False, action="store_true",
                       help="With --clusters: split every Louvain cluster into its connected pieces, so that no cluster is "
                            "two unrelated groups of cells; also write the connected components of the whole graph as "
                            "components.txt, one label per cell.")
    score.add_argument("--min-cluster-size", type=int, default=None, metavar="S",
                       help="With --clusters: merge every cluster of fewer than S cells into the cluster it shares the most "
                            "graph weight with. [0]")
    score.add_argument("--paga", default=False, action="store_true",
                       help="With --clusters: also write the cluster graph (PAGA) of the directed k-NN graph as "
                            "paga_connectivities.txt and paga_counts.txt (clusters x clusters).")
    score.add_argument("--pseudotime-root", type=int, nargs="+", default=None, metavar="I",
                       help="With --knn: also write the pseudotime of every cell from these root cells (one joint root set) "
                            "as pseudotime.txt: the shortest-path distance over the undirected k-NN distance graph to the "
                            "nearest root, divided by the largest finite one; inf for a cell no root reaches.")
    score.add_argument("--pseudotime-root-cluster", type=int, default=None, metavar="C",
                       help="With --clusters: the cells of cluster C are the root set of pseudotime.txt.")
    score.add_argument("--markers", default=False, action="store_true",
                       help="With -i and --clusters: also write the Wilcoxon rank-sum test of every gene, each cluster "
                            "against all the other cells, as marker_scores.txt and marker_pvals_adj.txt (genes x clusters); "
                            "with --genefile also ranked_markers.txt, the gene names by descending score per cluster.")
    score.add_argument("--marker-pairs", default=None, choices=["all", "neighbors"], metavar="WHICH",
                       help="With --markers: also write the rank-sum test of every gene between pairs of clusters, each pair "
                            "ranked alone -- all: every pair a < b; neighbors: the pairs with an edge of the k-NN graph between "
                            "them -- as pair_marker_pairs.txt (pairs x 2), pair_marker_scores.txt and "
                            "pair_marker_pvals_adj.txt (genes x pairs); with --genefile also ranked_pair_markers.txt.")
    score.add_argument("--pseudobulk", default=False, action="store_true",
                       help="With -i and --clusters and / or --sample-ids: also write the counts of every gene summed over the "
                            "cells of each group as pseudobulk_counts.txt (groups x genes, integers), the groups as "
                            "pseudobulk_groups.txt (one line per group: its keys and its cell count) and the fraction of "
                            "expressing cells as pseudobulk_pct.txt.")
    score.add_argument("--sample-ids", default=None, metavar="FILE",
                       help="With --pseudobulk: a text file with one sample id per cell; the groups are then sample x cluster "
                            "(or the samples alone without --clusters).")
    score.add_argument("--doublets", default=False, action="store_true",
                       help="With -i: also write Scrublet's doublet score of every cell, from simulated doublets projected "
                            "onto the model together with the cells (doublet_scores.txt: score, standard error and the "
                            "simulated rows among the neighbours, one row per cell; doublet_scores_sim.txt: score, "
                            "neighbours and the two parents of every simulated row).")
    score.add_argument("--doublet-ratio", type=float, default=None, metavar="R",
                       help="With --doublets: simulated rows per observed cell. [2.0]")
    score.add_argument("--doublet-rate", type=float, default=None, metavar="RHO",
                       help="With --doublets: the expected doublet rate. [0.06]")
    score.add_argument("--doublet-k", type=int, default=None, metavar="K",
                       help="With --doublets: neighbours before the adjustment for the simulated rows. "
                            "[round(0.5 sqrt(ncells))]")
    score.add_argument("--doublet-seed", type=int, default=None, metavar="S",
                       help="With --doublets: seed of the draw of the pairs. [0]")
    score.add_argument("--name-col", type=int, default=1, help="Zero-indexed column of --genefile with the names. [1]")

    proj = sub.add_parser("project", help="Project new cells onto a trained model.")
    proj.add_argument("-m", "--model", required=True, help="The model to project onto.")
    proj.add_argument("-i", "--input", required=True, help="Data to project (same formats as `train -i`).")
    proj.add_argument("-o", "--outdir", help="Output directory (default: the model's).")
    proj.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    proj.add_argument("--recalc-bp", action="store_true", help="Recompute the hyperparameter bp for the new data.")
    proj.add_argument("--max-iter", type=int, default=500, help="[500]")
    proj.add_argument("--min-iter", type=int, default=10, help="[10]")
    proj.add_argument("--epsilon", type=float, default=0.001, help="[0.001]")
    proj.add_argument("--check-freq", type=int, default=10, help="[10]")

    qc = sub.add_parser("qc", help="Per-cell and per-gene quality sums of a count matrix, and optionally the filtered "
                                   "matrix (this build's addition).")
    qc.add_argument("-i", "--input", required=True, help="The count matrix (same formats as `train -i`).")
    qc.add_argument("-o", "--outdir", help="Output directory (created if missing; default: the input's).")
    qc.add_argument("-p", "--prefix", default="", help="Prefix for output files.")
    qc.add_argument("--min-cells", type=float, default=0, metavar="M",
                    help="Keep genes observed in at least this many cells; a value in (0, 1) is a proportion of the cells. [0]")
    qc.add_argument("--min-genes", type=int, default=0, metavar="G", help="Keep cells with at least this many genes observed. [0]")
    qc.add_argument("--min-counts", type=int, default=0, metavar="C", help="Keep cells with at least this many counts. [0]")
    qc.add_argument("--max-counts", type=int, default=None, metavar="C", help="Keep cells with at most this many counts.")
    qc.add_argument("--gene-set", action="append", default=[], metavar="NAME=FILE",
                    help="A gene set whose counts are summed per cell (a column of cell_qc.txt): FILE holds one 0-based gene "
                         "index per line.  May be given up to 32 times.")
    qc.add_argument("--write-filtered", default=False, action="store_true",
                    help="Also write the filtered matrix (filtered.mtx) and the 0-based indices of the cells and genes it "
                         "keeps (kept_cells.txt, kept_genes.txt).")
    qc.add_argument("--n-top-genes", type=int, default=None, metavar="N",
                    help="Also select the N most variable genes by the variance of their Pearson residuals among the cells "
                         "and genes that pass the thresholds (gene_hvg.txt: residual variance, rank, 0/1 per gene; a gene "
                         "that fails --min-cells has nan, -1, 0).  With --write-filtered only the selected genes are kept.")
    qc.add_argument("--hvg-theta", type=float, default=None, metavar="T",
                    help="Overdispersion of the negative-binomial null of --n-top-genes; inf is the Poisson null. [100]")
    return parser


def _load_matrix(path):
    from .preprocessing import load_coo, load_mtx
    return load_mtx(path) if path.endswith(".mtx") else load_coo(path)


def _write_args(args, path):
    with open(path, "w") as fh:
        json.dump(args.__dict__, fh, indent=2)


def _write_matrix(path, X):
    from scipy.io import mmwrite
    mmwrite(path, X, field="integer")


def _prep(args, outprefix):
    """bin/scHPF:317-349: filtered.mtx, genes.txt, optionally the train / validation split."""
    from .preprocessing import load_and_filter, split_validation_cells
    filtered, genes = load_and_filter(args.input, min_cells=args.min_cells, whitelist=args.whitelist,
                                      blacklist=args.blacklist, filter_by_gene_name=args.filter_by_gene_name,
                                      no_split_on_dot=args.no_split_on_dot)
    print("Writing filtered data to file.....")
    _write_matrix("{}filtered.mtx".format(outprefix), filtered)
    genes.to_csv("{}genes.txt".format(outprefix), sep="\t", header=None, index=None)
    if args.n_validation_cells > 0:
        print("Selecting train/validation cells.....")
        Xtrn, Xvld, vld_ix = split_validation_cells(filtered, args.n_validation_cells, args.validation_group_ids,
                                                    max_group_frac=args.validation_max_group_frac)
        trn_ix = np.setdiff1d(np.arange(filtered.shape[0]), vld_ix)
        print("Writing train/validation splits.....")
        _write_matrix("{}train_cells.mtx".format(outprefix), Xtrn)
        np.savetxt("{}train_cell_ix.txt".format(outprefix), trn_ix, fmt="%d")
        _write_matrix("{}validation_cells.mtx".format(outprefix), Xvld)
        np.savetxt("{}validation_cell_ix.txt".format(outprefix), vld_ix, fmt="%d")
    print("Writing commandline arguments to file.....")
    _write_args(args, "{}prep_commandline_args.json".format(outprefix))


def _prep_like(args, outprefix):
    """bin/scHPF:353-366."""
    from .preprocessing import load_like
    print("Loading and reordering input like reference.... ")
    filtered, genes = load_like(args.input, reference=args.reference, by_gene_name=args.by_gene_name,
                                no_split_on_dot=args.no_split_on_dot)
    print("Writing prepared data to file.....")
    _write_matrix("{}filtered.mtx".format(outprefix), filtered)
    genes.to_csv("{}genes.txt".format(outprefix), sep="\t", header=None, index=None)
    print("Writing commandline arguments to file.....")
    _write_args(args, "{}prep-like_commandline_args.json".format(outprefix))


def _train(args, outprefix):
    from .trials import run_trials, run_trials_pool
    print("Loading data.....")
    train = _load_matrix(args.input)
    ncells, ngenes = train.shape
    print(".....found {} cells and {} genes in {}".format(ncells, ngenes, args.input))
    if args.batchsize and ncells > args.batchsize and not args.reproject:
        print("\nWARNING: running with minibatches but without reproject. We recommend adding the "
              "--reproject flag when running with batches to synchronize cell variational distributions. \n")
    vcells = None
    if args.validation_cells is not None:
        vcells = _load_matrix(args.validation_cells)
        print(".....found {} validation cells and {} genes in {}".format(vcells.shape[0], vcells.shape[1],
                                                                          args.validation_cells))
    thin_kwargs = {}
    if args.thin is not None:       # the split run_trials makes from the same (frac, seed), written out for reuse
        if vcells is not None:
            raise ValueError("--thin cannot be combined with --validation-cells")
        from .thinning import thin_counts
        print("Thinning counts (test fraction {}, seed {}).....".format(args.thin, args.thin_seed))
        thin_train, thin_test = thin_counts(train, args.thin, seed=args.thin_seed,
                                            device=args.devices[0] if args.devices else None)
        _write_matrix("{}thin_train.mtx".format(outprefix), thin_train)
        _write_matrix("{}thin_test.mtx".format(outprefix), thin_test)
        thin_kwargs = dict(thin=args.thin, thin_seed=args.thin_seed)
    print("Running trials.....")
    dtype = np.float32 if args.float32 else np.float64
    pooled = args.cmd != "train"
    if args.cmd == "train":
        run = run_trials
        if args.devices and len(args.devices) > 1:      # restarts spread over several GPUs
            run, pooled = partial(run_trials_pool, devices=args.devices, njobs=len(args.devices)), True
        elif args.devices:
            run = partial(run_trials, device=args.devices[0])
    else:
        if args.njobs < 0:
            raise ValueError("njobs must be an int >= 0, received {}".format(args.njobs))
        run = partial(run_trials_pool, njobs=args.njobs, devices=args.devices)
    result = run(train, vcells=vcells, nfactors=args.nfactors, ntrials=args.ntrials, min_iter=args.min_iter,
                 max_iter=args.max_iter, check_freq=args.check_freq, epsilon=args.epsilon,
                 better_than_n_ago=args.better_than_n_ago, dtype=dtype, verbose=args.verbose,
                 model_kwargs=dict(a=args.a, c=args.c), return_all=args.save_all, reproject=args.reproject,
                 batchsize=args.batchsize, beta_theta_simultaneous=args.beta_theta_simultaneous,
                 loss_smoothing=args.smooth_loss, **thin_kwargs)
    model, reject = result if args.save_all else (result, None)
    klist = [args.nfactors] if isinstance(args.nfactors, int) else args.nfactors
    if not pooled:                                      # run_trials: one model (and one list of rejects)
        model = [model]
        reject = [reject] if reject is not None else None
    for i, (K, m) in enumerate(zip(klist, model)):
        stem = "{}scHPF_K{}{}_{}trials".format(outprefix, K,
                                               "_b{}".format(args.batchsize) if ncells > args.batchsize else "",
                                               args.ntrials)
        if vcells is None:
            print("Saving best model ({} factors).....".format(K))
            joblib.dump(m, stem + ".joblib")
        else:
            print("Saving best model (training data, {} factors).....".format(K))
            joblib.dump(m, stem + ".train.joblib")
            print("Computing final validation projection ({} factors)....".format(K))
            joblib.dump(m.project(vcells, replace=False), stem + ".validation_proj.joblib")
        if args.save_all:
            for j, r in enumerate(reject[i]):
                joblib.dump(r, stem + "_reject{}.joblib".format(j + 1))
    if args.thin is None:
        del args.thin, args.thin_seed   # the arguments file of a run without thinning stays what it was
    cmdfile = "{}train_commandline_args.json".format(outprefix)
    if os.path.exists(cmdfile):
        cmdfile = "{}train_commandline_args.{}.json".format(outprefix, time.strftime("%Y%m%d-%H%M%S"))
    _write_args(args, cmdfile)


def _score(args, outprefix):
    from .util import max_pairwise_table, mean_cellscore_fraction_list
    if args.pseudobulk and not args.clusters and args.sample_ids is None:    # before anything is loaded or written
        raise ValueError("--pseudobulk needs groups: the clusters (--knn K --knn-graph M --clusters), --sample-ids FILE, or both")
    if args.sample_ids is not None and not args.pseudobulk:
        raise ValueError("--sample-ids belongs to --pseudobulk")
    if not args.clusters:
        for name in ("connected", "min_cluster_size", "paga"):
            if getattr(args, name):
                raise ValueError("--%s belongs to --clusters" % name.replace("_", "-"))
    if args.min_cluster_size is not None and args.min_cluster_size < 0:
        raise ValueError("--min-cluster-size must be >= 0")
    if args.pseudotime_root is not None and args.knn is None:
        raise ValueError("--pseudotime-root belongs to --knn")
    if args.pseudotime_root_cluster is not None and not args.clusters:
        raise ValueError("--pseudotime-root-cluster belongs to --clusters")
    if args.pseudotime_root is not None and args.pseudotime_root_cluster is not None:
        raise ValueError("--pseudotime-root and --pseudotime-root-cluster are two ways to name one root set: give one")
    labels = sample_ids = None
    print("Loading model.....")
    model = joblib.load(args.model)
    cell_score, gene_score = model.cell_score(), model.gene_score()
    print("Saving scores.....")
    np.savetxt(outprefix + "cell_score.txt", cell_score, delimiter="\t")
    np.savetxt(outprefix + "gene_score.txt", gene_score, delimiter="\t")
    with open(outprefix + "mean_cellscore_fraction.txt", "w") as fh:
        fh.write("nfactors\tmean_cellscore_fraction\n")
        for i, frac in enumerate(mean_cellscore_fraction_list(cell_score)):
            fh.write("{}\t{}\n".format(i + 1, frac))
    max_pairwise_table(gene_score, ntop_list=[50, 100, 150, 200, 250, 300, 350, 400, 450, 500]).to_csv(
        outprefix + "maximum_overlaps.txt", sep="\t", index=False)
    if args.genefile is not None:
        genes = np.loadtxt(args.genefile, delimiter="\t", dtype=str)
        if genes.ndim == 1:
            genes = genes[:, None]
        name_col = min(args.name_col, genes.shape[1] - 1)
        print(".....using {}'th column of genefile as gene label".format(name_col))
        ranks = np.argsort(gene_score, axis=0)[::-1]
        ranked = np.stack([genes[ranks[:, k], name_col] for k in range(gene_score.shape[1])]).T
        np.savetxt(outprefix + "ranked_genes.txt", ranked, fmt="%s", delimiter="\t")
    if args.input is not None:
        from . import loss as ls
        print("Loading data.....")
        data = _load_matrix(args.input)
        if tuple(data.shape) != (model.theta.dims[0], model.beta.dims[0]):
            raise ValueError("{} is {} x {}, the model was fitted to {} cells x {} genes".format(
                args.input, data.shape[0], data.shape[1], model.theta.dims[0], model.beta.dims[0]))
        if args.sample_ids is not None:
            with open(args.sample_ids) as fh:
                sample_ids = np.array([line.rstrip("\r\n") for line in fh], dtype=str)
            if len(sample_ids) != data.shape[0]:
                raise ValueError("{} holds {} sample ids, the matrix has {} cells".format(args.sample_ids, len(sample_ids),
                                                                                         data.shape[0]))
        print("Saving per-cell and per-gene loss.....")
        np.savetxt(outprefix + "cell_loss.txt", ls.cellmean_negative_pois_llh(data, theta=model.theta, beta=model.beta))
        np.savetxt(outprefix + "gene_loss.txt", ls.genemean_negative_pois_llh(data, theta=model.theta, beta=model.beta))
        if args.ppc:
            print("Saving posterior predictive checks.....")
            for by in ("gene", "cell"):
                ppc = ls.predictive_check(data, theta=model.theta, beta=model.beta, by=by)
                np.savetxt(outprefix + by + "_ppc.txt", np.stack([ppc[c] for c in ls.PPC_COLUMNS], axis=1))
    else:
        if args.ppc:
            raise ValueError("--ppc needs the count matrix (-i)")
        if args.markers:
            raise ValueError("--markers needs the count matrix (-i)")
        if args.doublets:
            raise ValueError("--doublets needs the count matrix (-i)")
        if args.pseudobulk:
            raise ValueError("--pseudobulk needs the count matrix (-i)")
        del args.input  # the arguments file of a run without the matrix stays what it was
    if not args.ppc:
        del args.ppc     # ... and so does the arguments file of a run without the check
    if args.knn is not None:
        print("Saving nearest neighbours.....")
        indices, distances = model.neighbors(k=args.knn, metric=args.knn_metric)
        np.savetxt(outprefix + "knn_indices.txt", indices, fmt="%d", delimiter="\t")
        np.savetxt(outprefix + "knn_distances.txt", distances, delimiter="\t")
        if args.knn_graph is not None:
            from scipy.io import mmwrite
            from .neighbors import knn_connectivities, louvain
            graph = knn_connectivities(indices, distances, method=args.knn_graph)
            mmwrite(outprefix + "knn_connectivities.mtx", graph)
            if args.clusters:
                print("Saving clusters.....")
                args.resolution = 1.0 if args.resolution is None else args.resolution
                labels = louvain(graph, resolution=args.resolution, connected=args.connected)
                if args.connected:
                    from .topology import connected_components
                    np.savetxt(outprefix + "components.txt", connected_components(graph), fmt="%d")
                if args.min_cluster_size:
                    from .topology import absorb_small, cluster_graph
                    table = cluster_graph(graph, labels)
                    labels = absorb_small(labels, table["weight"], table["n_cells"], args.min_cluster_size)[0]
                np.savetxt(outprefix + "clusters.txt", labels, fmt="%d")
                if args.paga:
                    from .neighbors import knn_graph
                    from .topology import paga
                    print("Saving the cluster graph.....")
                    found = paga(knn_graph(indices, distances, indices.shape[0]), labels)
                    np.savetxt(outprefix + "paga_connectivities.txt", found["connectivities"], delimiter="\t")
                    np.savetxt(outprefix + "paga_counts.txt", found["count"], fmt="%d", delimiter="\t")
                if args.markers:
                    from .markers import rank_genes_groups
                    print("Saving marker genes.....")
                    found = rank_genes_groups(data, labels)
                    np.savetxt(outprefix + "marker_scores.txt", found["scores"].T, delimiter="\t")
                    np.savetxt(outprefix + "marker_pvals_adj.txt", found["pvals_adj"].T, delimiter="\t")
                    if args.genefile is not None:
                        ranks = np.argsort(found["scores"].T, axis=0)[::-1]
                        ranked = np.stack([genes[ranks[:, c], name_col] for c in range(ranks.shape[1])]).T
                        np.savetxt(outprefix + "ranked_markers.txt", ranked, fmt="%s", delimiter="\t")
                    if args.marker_pairs is not None:
                        from .markers import rank_genes_pairs
                        print("Saving pairwise marker genes.....")
                        pairs = args.marker_pairs
                        if pairs == "neighbors":
                            from .neighbors import knn_graph
                            from .topology import paga
                            count = np.asarray(paga(knn_graph(indices, distances, indices.shape[0]), labels)["count"])
                            pairs = np.stack(np.nonzero(np.triu((count + count.T) > 0, 1)), axis=1).astype(np.int32)
                        found = rank_genes_pairs(data, labels, pairs=pairs)
                        np.savetxt(outprefix + "pair_marker_pairs.txt", found["pairs"].reshape(-1, 2), fmt="%d", delimiter="\t")
                        np.savetxt(outprefix + "pair_marker_scores.txt", found["scores"].T, delimiter="\t")
                        np.savetxt(outprefix + "pair_marker_pvals_adj.txt", found["pvals_adj"].T, delimiter="\t")
                        if args.genefile is not None:
                            ranked = genes[:, name_col][np.argsort(found["scores"].T, axis=0)[::-1]]   # genes x pairs
                            np.savetxt(outprefix + "ranked_pair_markers.txt", ranked, fmt="%s", delimiter="\t")
        root = args.pseudotime_root
        if args.pseudotime_root_cluster is not None and labels is not None:
            root = np.asarray(labels) == args.pseudotime_root_cluster
            if not root.any():
                raise ValueError("--pseudotime-root-cluster {}: no cell is in that cluster".format(args.pseudotime_root_cluster))
        if root is not None:
            from .neighbors import knn_graph
            from .paths import pseudotime
            print("Saving pseudotime.....")
            np.savetxt(outprefix + "pseudotime.txt", pseudotime(knn_graph(indices, distances, indices.shape[0]), root))
    else:
        if args.knn_graph is not None:
            raise ValueError("--knn-graph needs the neighbour lists (--knn K)")
        del args.knn, args.knn_metric   # ... and of a run without the neighbours
    if args.knn_graph is None:
        if args.clusters:
            raise ValueError("--clusters needs the neighbour graph (--knn K --knn-graph M)")
        del args.knn_graph              # ... and without their graph
    if not args.clusters:
        if args.resolution is not None:
            raise ValueError("--resolution belongs to --clusters")
        if args.markers:
            raise ValueError("--markers needs the clusters (--knn K --knn-graph M --clusters)")
        del args.clusters, args.resolution   # ... and without its clusters
    for name in ("connected", "min_cluster_size", "paga"):
        if not getattr(args, name):
            delattr(args, name)              # ... or their connected pieces, merged splinters and cluster graph
    for name in ("pseudotime_root", "pseudotime_root_cluster"):
        if getattr(args, name) is None:
            delattr(args, name)              # ... or a pseudotime
    if args.marker_pairs is not None and not args.markers:
        raise ValueError("--marker-pairs needs the marker genes (-i X --knn K --knn-graph M --clusters --markers)")
    if not args.markers:
        del args.markers                     # ... and without their marker genes
    if args.marker_pairs is None:
        del args.marker_pairs                # ... or the genes between pairs of clusters
    if args.pseudobulk:
        from .aggregate import pseudobulk
        print("Saving pseudobulk.....")
        found = pseudobulk(data, tuple(key for key in (sample_ids, labels) if key is not None))
        np.savetxt(outprefix + "pseudobulk_counts.txt", found["counts"], fmt="%d", delimiter="\t")
        np.savetxt(outprefix + "pseudobulk_pct.txt", found["pct"], delimiter="\t")
        with open(outprefix + "pseudobulk_groups.txt", "w") as fh:
            for keys, n in zip(found["groups"], found["n_cells"]):
                fh.write("\t".join([str(k) for k in keys] + [str(int(n))]) + "\n")
    else:
        del args.pseudobulk, args.sample_ids   # ... or a pseudobulk table
    if args.doublets:
        from .doublets import doublet_scores
        print("Saving doublet scores.....")
        args.doublet_ratio = 2.0 if args.doublet_ratio is None else args.doublet_ratio
        args.doublet_rate = 0.06 if args.doublet_rate is None else args.doublet_rate
        args.doublet_seed = 0 if args.doublet_seed is None else args.doublet_seed
        found = doublet_scores(model, data, ratio=args.doublet_ratio, expected_rate=args.doublet_rate, k=args.doublet_k,
                               seed=args.doublet_seed, verbose=False)
        np.savetxt(outprefix + "doublet_scores.txt", np.stack([found["scores"], found["se"], found["k_sim"]], axis=1),
                   delimiter="\t", header="score\tse\tk_sim")
        np.savetxt(outprefix + "doublet_scores_sim.txt",
                   np.concatenate([np.stack([found["scores_sim"], found["k_sim_sim"]], axis=1), found["parents"]], axis=1),
                   delimiter="\t", header="score\tk_sim\tparent_a\tparent_b")
    else:
        for name in ("doublet_ratio", "doublet_rate", "doublet_k", "doublet_seed"):
            if getattr(args, name) is not None:
                raise ValueError("--%s belongs to --doublets" % name.replace("_", "-"))
        del args.doublets, args.doublet_ratio, args.doublet_rate, args.doublet_k, args.doublet_seed   # ... or doublet scores
    _write_args(args, "{}score_commandline_args.json".format(outprefix))


def _project(args, outprefix):
    print("Loading reference model.....")
    model = joblib.load(args.model)
    print("Loading data.....")
    data = _load_matrix(args.input)
    print("Projecting data.....")
    projection = model.project(data, replace=False, verbose=True, recalc_bp=args.recalc_bp,
                               min_iter=args.min_iter, max_iter=args.max_iter, check_freq=args.check_freq,
                               epsilon=args.epsilon)
    if args.recalc_bp:
        outprefix += "recalc_bp."
    joblib.dump(projection, "{}{}.proj.joblib".format(outprefix, args.model.rsplit(".", 1)[0].split("/")[-1]))
    _write_args(args, "{}project_commandline_args.json".format(outprefix))


def _qc(args, outprefix):
    from .qc import filter_counts
    print("Loading data.....")
    data = _load_matrix(args.input)
    gene_sets = {}
    for spec in args.gene_set:
        name, sep, path = spec.partition("=")
        if not sep or not name or not path:
            raise ValueError("--gene-set takes NAME=FILE, got {}".format(spec))
        gene_sets[name] = np.loadtxt(path, dtype=np.int64, ndmin=1)
    print("Computing quality sums.....")
    filtered, cell_keep, gene_keep, found = filter_counts(data, min_cells=args.min_cells, min_genes=args.min_genes,
                                                          min_counts=args.min_counts, max_counts=args.max_counts,
                                                          gene_sets=gene_sets)
    names = list(gene_sets)
    np.savetxt(outprefix + "cell_qc.txt",
               np.stack([found["cell_n_genes"], found["cell_total"]] + [found["cell_set_total"][n] for n in names], axis=1),
               fmt="%d", delimiter="\t", header="\t".join(["n_genes", "total"] + names), comments="")
    with open(outprefix + "gene_qc.txt", "w") as fh:
        fh.write("n_cells\ttotal\tsumsq\tmean\tvar\n")
        for j in range(len(found["gene_n_cells"])):
            fh.write("{}\t{}\t{}\t{!r}\t{!r}\n".format(found["gene_n_cells"][j], found["gene_total"][j], found["gene_sumsq"][j],
                                                     float(found["gene_mean"][j]), float(found["gene_var"][j])))
    print(".....{} of {} cells and {} of {} genes pass".format(int(cell_keep.sum()), len(cell_keep), int(gene_keep.sum()),
                                                                len(gene_keep)))
    if args.n_top_genes is not None:
        from .qc import submatrix
        from .variable_genes import highly_variable_genes
        print("Selecting variable genes.....")
        args.hvg_theta = 100.0 if args.hvg_theta is None else args.hvg_theta
        hvg = highly_variable_genes(filtered, n_top_genes=args.n_top_genes, theta=args.hvg_theta)
        kept = np.flatnonzero(gene_keep)       # the genes that fail --min-cells are out before the ranking
        var, rank, chosen = np.full(len(gene_keep), np.nan), np.full(len(gene_keep), -1, np.int64), np.zeros(len(gene_keep), bool)
        var[kept], rank[kept], chosen[kept] = hvg["residual_var"], hvg["rank"], hvg["highly_variable"]
        with open(outprefix + "gene_hvg.txt", "w") as fh:
            fh.write("residual_var\trank\thighly_variable\n")
            for j in range(len(gene_keep)):
                fh.write("{!r}\t{}\t{}\n".format(float(var[j]), rank[j], int(chosen[j])))
        print(".....{} of {} genes selected".format(int(chosen.sum()), len(chosen)))
        filtered, gene_keep = submatrix(filtered, genes=hvg["highly_variable"]), chosen
    else:
        if args.hvg_theta is not None:
            raise ValueError("--hvg-theta belongs to --n-top-genes")
        del args.n_top_genes, args.hvg_theta         # the arguments file is what it was without the selection
    if args.write_filtered:
        print("Writing filtered data to file.....")
        _write_matrix(outprefix + "filtered.mtx", filtered)
        np.savetxt(outprefix + "kept_cells.txt", np.flatnonzero(cell_keep), fmt="%d")
        np.savetxt(outprefix + "kept_genes.txt", np.flatnonzero(gene_keep), fmt="%d")
    _write_args(args, "{}qc_commandline_args.json".format(outprefix))


def main(argv=None):
    parser = _parser()
    args = parser.parse_args(argv)
    if args.cmd is None:
        parser.print_help(sys.stderr)
        return 1
    if args.outdir is None:     # the reference's defaults (bin/scHPF:305-311)
        if args.cmd in ("prep", "prep-like", "train", "train-pool", "qc"):
            args.outdir = args.input.rsplit("/", 1)[0] if "/" in args.input else "."
        elif args.cmd == "project":
            args.outdir = args.model.rsplit("/", 1)[0] if "/" in args.model else "."
        else:
            args.outdir = args.model.split(".joblib")[0]
    if not os.path.exists(args.outdir):
        print("Creating output directory {} ".format(args.outdir))
        os.makedirs(args.outdir)
    prefix = args.prefix.rstrip(".") + "." if args.prefix else ""
    outprefix = args.outdir + "/" + prefix
    {"prep": _prep, "prep-like": _prep_like, "train": _train, "train-pool": _train, "score": _score,
     "project": _project, "qc": _qc}[args.cmd](args, outprefix)
    return 0


if __name__ == "__main__":
    sys.exit(main())
