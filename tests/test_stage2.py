"""CPU: rambl.py stage 2 (gene abundance, gene_abundance.py) -- a hand-computed depth file, the plain restatement of the
contract (a loop in pure Python, below) on seeded random depth files printed by stage1.bed_text, the two corners the
module decides, and the command line."""
import random
from fractions import Fraction

import pytest

from rambl_amd import stage1, stage2


def _files(tmp_path, bed, index):
    d, gi = str(tmp_path / "gene_depth.txt"), str(tmp_path / "genes.fai")
    open(d, "w").write(bed)
    open(gi, "w").write("".join("%s\t%d\t0\t60\t61\n" % r for r in index))
    return d, gi


def test_hand_computed_depth_file(tmp_path):
    # gA is 100 bases long, gB 50.  Stage 1 found on gA positions 3-26 (24 positions, depth sum 28) and 38-40 (3 positions,
    # depth sum 3), on gB positions 10-30 (20 of them covered, depth sum 50); then gA comes back with 50-60 at depth 4.
    #   gA 3 27 1.1667   breadth (27 - 3 + 1) / 100 = 0.25: the 24 positions count 25, as `end` is last position + 1
    #                    depth 1.1667: the printed mean, not 28 / 24 = 1.16666...
    #   gA 38 41 1       breadth 0.04, depth 1
    #     -> abundance 0.25 * 1.1667 + 0.04 * 1 = 0.291675 + 0.04 = 0.331675   (from the exact mean: 0.331667)
    #        ratio 0.25 + 0.04 = 0.29
    #   gB 10 31 2.5     breadth 22 / 50 = 0.44 -> abundance 1.1, ratio 0.44
    #   gA 50 61 4       a name that returns starts a new group: breadth 0.12 -> abundance 0.48, ratio 0.12
    bed = stage1.bed_text([("gA", 3, 26, 28, 24), ("gA", 38, 40, 3, 3)]) + stage1.bed_text([("gB", 10, 30, 50, 20), ("gA", 50, 60, 44, 11)])
    assert bed == "gA\t3\t27\t1.1667\ngA\t38\t41\t1\ngB\t10\t31\t2.5\ngA\t50\t61\t4\n"
    d, gi = _files(tmp_path, bed, [("gA", 100), ("gB", 50), ("gC", 70)])
    assert stage2.gene_abundance(d, gi) == ["gA\t1\t100\t0.331675\t0.290000", "gB\t1\t50\t1.100000\t0.440000",
                                            "gA\t1\t100\t0.480000\t0.120000"]           # gC has no row: not printed


def test_rows_without_depth_do_not_count_as_covered(tmp_path):
    # g: 200 bases; rows 1-50 at mean 0 (breadth 0.255) and 101-120 at mean 3 (breadth 0.105): abundance 0.315, ratio 0.105
    d, gi = _files(tmp_path, "g\t1\t51\t0\ng\t101\t121\t3\n", [("g", 200)])
    assert stage2.gene_abundance(d, gi) == ["g\t1\t200\t0.315000\t0.105000"]


def _restated(depth_path, index_path):
    """The contract as a plain loop: runs of equal names, breadth (end - start + 1) / length, abundance the sum of
    breadth x depth, ratio the sum of the breadths with depth above 0.

    The abundance is accumulated left to right with one rounding per row (a fused multiply-add, done here in exact
    rationals), not with `abun += b * a`.  That is what numpy's dot computes for a gene's handful of rows: it calls the
    BLAS ddot, whose scalar loop (vectors of fewer than 32 elements) is compiled to fused multiply-adds on every x86-64
    CPU with FMA3, which any host of an MI355X has.  The difference is one unit in the last place of the double, and it
    shows in the printed `%f` more often than chance would have it: a five-digit mean times k / 1200 is a short decimal,
    so sums such as 0.3175 x 40.063 + 0.03 x 625.14 = 31.4742025 lie exactly on a rounding boundary of the sixth decimal
    (two of the thousand groups below), where the twice-rounded loop prints 31.474202 and numpy 31.474203."""
    length = {}
    for line in open(index_path):
        f = line.rstrip("\n").split("\t")
        length[f[0]] = int(f[1])
    rows = [line.rstrip("\n").split("\t") for line in open(depth_path)]
    out, i = [], 0
    while i < len(rows):
        name = rows[i][0]
        abun, ratio = 0.0, 0
        while i < len(rows) and rows[i][0] == name:
            b = (float(rows[i][2]) - float(rows[i][1]) + 1.0) / length[name]
            a = float(rows[i][3])
            abun = float(Fraction(abun) + Fraction(b) * Fraction(a))
            if a > 0:
                ratio += b
            i += 1
        out.append("%s\t%d\t%d\t%f\t%f" % (name, 1, length[name], abun, ratio))
    return out


@pytest.mark.parametrize("seed", range(8))
def test_random_depth_files_match_the_restatement(seed, tmp_path):
    rng = random.Random(2000 + seed)
    index = [("%d" % (4000000 + k), rng.choice([900, 1200, 1500, 1501])) for k in range(rng.choice([3, 40, 300]))]
    iv = []
    for name, ln in index:
        if rng.random() < 0.3:
            continue
        p = 1
        for _ in range(rng.randint(1, 6)):
            s = p + rng.randint(0, 300)
            e = s + rng.randint(0, 400)
            if e > ln:
                break
            n = rng.randint(1, e - s + 1)                     # covered positions of the interval (gaps of up to 10 inside)
            iv.append((name, s, e, n * rng.randint(1, 40) + rng.randint(0, 6000), n))
            p = e + 12
    if seed % 2:                                               # file order is the order of the groups: some names come back
        rng.shuffle(iv)
    d, gi = _files(tmp_path, stage1.bed_text(iv), index)
    got = stage2.gene_abundance(d, gi)
    assert got == _restated(d, gi)
    assert len(got) >= len({r[0] for r in iv}) > 0


def test_empty_depth_file_and_unknown_gene(tmp_path):
    d, gi = _files(tmp_path, "", [("g", 100)])
    assert stage2.gene_abundance(d, gi) == []
    d, gi = _files(tmp_path, "g\t1\t11\t2\nh77\t1\t11\t2\n", [("g", 100)])
    with pytest.raises(ValueError, match="h77"):
        stage2.gene_abundance(d, gi)


def test_command_line(tmp_path, capsys):
    d, gi = _files(tmp_path, "g\t1\t11\t2\n", [("g", 100)])
    assert stage2.main(["-v", d, gi]) == 0
    assert capsys.readouterr().out == "g\t1\t100\t0.220000\t0.110000\n"
    d, gi = _files(tmp_path, "h77\t1\t11\t2\n", [("g", 100)])
    assert stage2.main([d, gi]) == 1
    cap = capsys.readouterr()
    assert cap.out == "" and "h77" in cap.err
