"""Stage 2 of rambl.py: gene abundance and coverage ratio from stage 1's intervals.

Mirror of scripts/gene_abundance.py:45-88 (`gene_abundance.py [-v] DEPTH GENE_INDEX`, launched by rambl.py:105-119): the
rows of the depth file (stage 1's BED text: name, start, end, mean depth) are grouped by runs of equal name in file order
-- a name that comes back after another gene starts a new group and is printed again --, a row's breadth is
`(end - start + 1) / gene length` with `end` as stage 1 prints it (last position + 1, so a row of n positions counts
n + 1), its depth the printed mean; a group's abundance is `numpy.dot(breadth ** 1.0, depth)`, its coverage ratio the sum
of the breadths of the rows with a depth above 0; one line `name <TAB> 1 <TAB> length <TAB> abundance <TAB> ratio` per
group.  Genes without rows are not printed.

This stage stays on the host and reads text on purpose.  The depth the reference's stage 3 sees is `float()` of the mean as
printed, five significant digits, not the exact depth sum / covered positions stage 1 holds on the device: an abundance
computed there from the exact sums would be another number, and a clade next to a threshold of stage 3 another seed
list.  The work is one multiply-add per interval.  The abundance is numpy's `dot`, as in the script: a five-digit mean
times k / gene length is a short decimal, sums of them fall exactly on a rounding boundary of the printed `%f` now and
then, and there the last digit is the one the BLAS behind `dot` gives (fused multiply-adds), not that of a Python loop.

Two corners the reference script handles by accident are decided here: an empty depth file gives no output (the script
prints a line for gene `None`), and a gene of the depth file that the index does not hold is an error that names it
(the script divides by the 0 of its defaultdict).
"""
import sys

import numpy as np


def read_index(index_path):
    """{name: length} from columns 1-2 of the gene index (.fai); a name listed twice keeps its last length (:53-57)."""
    size = {}
    with open(index_path) as f:
        for line in f:
            row = line.rstrip("\r\n").split("\t")
            if len(row) > 1:
                size[row[0]] = int(row[1])
    return size


def _group_line(name, length, breadth, depth):
    abun = np.dot(np.power(breadth, 1.0), depth)              # cal_gene_abundance, :22-35
    ratio = sum(r for r, a in zip(breadth, depth) if a > 0)   # cal_gene_coverage, :37-43: left to right
    return "%s\t%d\t%d\t%f\t%f" % (name, 1, length, abun, ratio)


def gene_abundance(depth_path, index_path):
    """-> the lines gene_abundance.py prints (without the newline), one per run of rows of one gene."""
    size = read_index(index_path)
    lines = []
    name, breadth, depth = None, [], []
    with open(depth_path) as f:
        for line in f:
            row = line.rstrip("\r\n").split("\t")
            if row == [""]:
                continue
            if name is not None and name != row[0]:
                lines.append(_group_line(name, size[name], breadth, depth))
                breadth, depth = [], []
            name = row[0]
            if name not in size:
                raise ValueError("gene %s of %s is not in the gene index %s" % (name, depth_path, index_path))
            breadth.append((float(row[2]) - float(row[1]) + 1.) / size[name])
            depth.append(float(row[3]))
    if name is not None:
        lines.append(_group_line(name, size[name], breadth, depth))
    return lines


def main(argv=None):
    """`python -m rambl_amd.stage2 [-v] DEPTH GENE_INDEX`: the argv and the stdout of gene_abundance.py."""
    import argparse
    import logging
    import os
    ap = argparse.ArgumentParser(description="Calculate gene abundance (rambl.py stage 2)")
    ap.add_argument("cov", metavar="DEPTH", help="gene depth file")
    ap.add_argument("gi", metavar="GENE", help="gene index file")
    ap.add_argument("-v", dest="verbose", action="store_true", help="verbose output")
    a = ap.parse_args(argv)
    logging.basicConfig(format="[%(asctime)s] %(levelname)s : %(message)s", level=logging.INFO)
    if a.verbose:
        logging.info("process records in %s with the gene info of %s", os.path.abspath(a.cov), os.path.abspath(a.gi))
    try:
        lines = gene_abundance(a.cov, a.gi)
    except ValueError as e:
        sys.stderr.write("stage2: %s\n" % e)
        return 1
    sys.stdout.write("".join(ln + "\n" for ln in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
