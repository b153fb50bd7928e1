"""Do consecutive master steps overlap?  From a rocprofv3 results .db (kernel-trace) of back-to-back steps: per step
(one k_analyze launch to the next), the microseconds in which no kernel runs, in which only the small kernels run (the
FIR-design chain, the filter spectra, the level-correction tail) and in which a big kernel runs; and which kernels of
step k the analysis of step k + 1 runs under.

    python tools/pipeline_timeline.py results.db
"""
import sqlite3
import sys

SMALL = ("k_match_curve", "k_profile_curve", "k_fir_", "k_conv_wide_prep", "k_conv_prep", "k_correction_tail", "k_levels",
         "k_average_spectra")


def short(name):
    return name.split("(")[0].replace("void mgx::", "").replace("mgx::", "")[:40]


def main():
    cur = sqlite3.connect(sys.argv[1]).cursor()
    rows = [(n, s, e) for n, s, e in cur.execute("select name, start, end from kernels order by start").fetchall()
            if "k_" in n]
    firsts = [i for i, r in enumerate(rows) if "k_analyze" in r[0]]
    limits = [r for r in rows if "k_limit" in r[0]]                # the k-th limiter launch belongs to the k-th analysis
    if len(firsts) < 3:
        print("fewer than three steps found")
        return
    print("%4s %9s %9s %9s %9s   %s" % ("step", "period", "idle", "small", "big", "the next step's k_analyze starts ... and runs beside"))
    for k in range(len(firsts) - 1):
        t0, t1 = rows[firsts[k]][1], rows[firsts[k + 1]][1]
        marks = sorted({t0, t1} | {t for _, s, e in rows for t in (s, e) if t0 < t < t1})
        idle = small = big = 0.0
        for a, b in zip(marks, marks[1:]):
            live = [n for n, s, e in rows if s <= a and e >= b]
            span = (b - a) / 1e3
            if not live:
                idle += span
            elif all(any(x in n for x in SMALL) for n in live):
                small += span
            else:
                big += span
        an, as_, ae = rows[firsts[k + 1]]
        under = ["%s %.1f us" % (short(n), (min(e, ae) - max(s, as_)) / 1e3)
                 for i, (n, s, e) in enumerate(rows) if i != firsts[k + 1] and s < ae and e > as_]
        ahead = "%.1f us before this step's k_limit ends; " % ((limits[k][2] - as_) / 1e3) if k < len(limits) else ""
        print("%4d %9.1f %9.1f %9.1f %9.1f   %s%s" % (k, (t1 - t0) / 1e3, idle, small, big, ahead, ", ".join(under) or "nothing"))


if __name__ == "__main__":
    main()
