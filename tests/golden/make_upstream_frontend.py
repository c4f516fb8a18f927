"""Record tests/golden/upstream_frontend.json for tests/test_upstream_frontend.py (no GPU needed, the library built).

    python tests/golden/make_upstream_frontend.py COMMIT [OUT.json]
    python tests/golden/make_upstream_frontend.py --coverage

Run it on a checkout of the commit whose behaviour is to be kept, with that commit's library built; COMMIT is stored in
the file as `commit`.  The cases, inputs and harness are the test module's own (`tables`, `record_of`), so generator and
test cannot drift.  The file holds data only: case ids, exception type names and messages, and the hex digest of
every other case's record (the entry called, its typed scalars, the dtypes, shapes and digests of its arrays, and the
same of what the callable returned).  A refactor of `ssqueeze_rs_amd/upstream.py` does NOT regenerate it.

Either form ends with the coverage of the table: every `raise` and `assert` statement of upstream.py, and which of them
no case of the table was raised from (`--coverage` prints that alone and writes nothing).
"""
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_upstream_frontend as t  # noqa: E402


def raise_lines():
    with open(t.up.__file__) as f:
        tree = ast.parse(f.read())
    return sorted(n.lineno for n in ast.walk(tree) if isinstance(n, (ast.Raise, ast.Assert)))


def main():
    only_coverage = sys.argv[1:] == ["--coverage"]
    lines, cases = [], {}
    for cid in t.case_ids():
        cases[cid] = t.record_of(cid, lines)
    accepted = {cid: t.outcome(cases[cid]) for cid in t.tables().accepted}
    refused = {}
    for cid in t.tables().refusals:
        refused.setdefault(t.outcome(cases[cid]), []).append(cid)
    hit = set(lines)
    stmts = raise_lines()
    missed = [n for n in stmts if n not in hit]
    n_refused = sum("raises" in c or "raises" in c.get("then", {}) for c in cases.values())
    print(f"{len(cases)} cases, {n_refused} of them refused; {len(stmts) - len(missed)} of the {len(stmts)} raise / "
          f"assert statements of upstream.py are reached; not reached: lines {missed}")
    if only_coverage:
        return
    commit = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else t.GOLDEN
    with open(dst, "w") as f:
        f.write('{"commit": %s,\n "accepted": {\n' % json.dumps(commit))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in accepted.items()))
        f.write('\n },\n "refused": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in refused.items()))
        f.write("\n }\n}\n")
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes, commit {commit}")


if __name__ == "__main__":
    main()
