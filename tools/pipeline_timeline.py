"""Do consecutive master steps overlap?  From a rocprofv3 results .db (kernel-trace) of back-to-back steps: per step
(one k_analyze launch to the next), the microseconds in which no kernel runs, in which only the small kernels run (the
FIR-design chain, the filter spectra, the level-correction tail) and in which a big kernel runs; and which kernels of
step k the analysis of step k + 1 runs under.  Then, per launch of k_correction_tail -- the one stretch of a
step's back half that leaves most of the chip idle -- which kernels run while it runs and for how long, and how long after
its end the step's k_limit starts (the context is released behind round 0, so the analysis of the step after next
belongs there).

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
    tails = [r for r in rows if "k_correction_tail" in r[0]]
    print()
    print("%4s %9s %9s %9s %9s   %s" % ("tail", "runs", "conv", "round 0", "-> limit", "beside the tail"))
    for k, (_, ts, te) in enumerate(tails):
        beside = ["%s %.1f us%s" % (short(n), (min(e, te) - max(s, ts)) / 1e3,
                                   " (starts %+.1f us from the tail's start)" % ((s - ts) / 1e3) if "k_analyze" in n else "")
                  for n, s, e in rows if (s, e) != (ts, te) and s < te and e > ts]
        # the convolution and round 0 of the same step: the last of each that started before this tail
        conv = [(e - s) / 1e3 for n, s, e in rows if "k_conv" in n and "prep" not in n and s < ts]
        round0 = [(e - s) / 1e3 for n, s, e in rows if "k_correction_round" in n and s < ts]
        limit = [(s - te) / 1e3 for n, s, e in rows if "k_limit" in n and s >= ts]
        print("%4d %9.1f %9s %9s %9s   %s" % (k, (te - ts) / 1e3, "%.1f" % conv[-1] if conv else "-",
                                             "%.1f" % round0[-1] if round0 else "-", "%+.1f" % limit[0] if limit else "-",
                                             ", ".join(beside) or "nothing"))


if __name__ == "__main__":
    main()
