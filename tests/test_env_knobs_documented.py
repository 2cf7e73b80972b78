"""The README's "Environment knobs of the KMeans engine" paragraph lists exactly the CML_KMEANS_* / CML_DELTA_*
variables the package reads, and nothing retired is left in the package."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "clustermachinelearningforhospitalnetworks_apache_spark_amd")
SOURCES = ("models/kmeans.py", "models/kmeans_route.py", "models/kmeans_init.py", "models/kmeans_prune_host.py",
           "models/kmeans_layout.py", "ops/kmeans_ops.py", "ml/clustering.py")
NAME = r"CML_(?:KMEANS|DELTA)_[A-Z0-9_]+"
# knobs, hooks and state of the A/B paths that lost their measurements (README, "Retired knobs and paths")
RETIRED = ("CML_KMEANS_SPLIT_FULL", "CML_KMEANS_OVERLAP_ROWS", "CML_KMEANS_SEED_UB", "CML_KMEANS_LAZY_BOUNDS",
           "CML_KMEANS_FUSED_TAIL", "CML_DELTA_FUSED_FIXUP", "set_assign_sched", "g_assign_sched",
           "set_delta_fused_fixup", "split_steps", "_seed_ub", "_full_split", "_overlap_split", "_msgs_split",
           "_msgs2", "_hist2", "g_mn_f32", "g_mn_no16", "multinomial_mfma_kernel", "PACK4")


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


def test_readme_lists_exactly_the_variables_the_package_reads():
    # (kmeans_route.py reads the knobs from the mapping it is given, ``env``: os.environ in the engine)
    env_read = re.compile(r"\b(?:os\.environ|env)(?:\.get)?\s*[\(\[]\s*[\"'](" + NAME + r")[\"']")
    read = set()
    for rel in SOURCES:
        read |= set(env_read.findall(_read(os.path.join(PKG, rel))))
    assert len(read) > 10, read  # the expression still finds the reads
    readme = _read(os.path.join(ROOT, "README.md"))
    start = readme.index("- Environment knobs of the KMeans engine")
    para = readme[start:readme.index("\n- ", start)]
    named = set(re.findall(NAME, para))
    assert named == read, {"undocumented": sorted(read - named), "documented but not read": sorted(named - read)}


def test_no_retired_name_left_in_the_package():
    left = []
    for base, dirs, files in os.walk(PKG):
        dirs[:] = [d for d in dirs if d not in ("__pycache__", "build")]
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = _read(os.path.join(base, f))
                left += [(os.path.relpath(os.path.join(base, f), ROOT), name) for name in RETIRED if name in text]
    assert not left, left
