#!/usr/bin/env python3
"""Code lines of Python files: non-blank, non-comment lines, docstrings of modules, classes and functions excluded.
    python tools/sloc.py FILE...          (git show REV:FILE > /tmp/x.py for another revision's)"""
import ast
import sys
import tokenize

SKIP = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENDMARKER)


def sloc(path: str) -> int:
    doc, code = set(), set()
    for n in ast.walk(ast.parse(open(path).read())):
        if isinstance(n, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(n, clean=False) is not None:
            doc.update(range(n.body[0].lineno, n.body[0].end_lineno + 1))
    with open(path) as f:
        for t in tokenize.generate_tokens(f.readline):
            if t.type not in SKIP:
                code.update(range(t.start[0], t.end[0] + 1))
    return len(code - doc)


if __name__ == "__main__":
    counts = [(sloc(p), p) for p in sys.argv[1:]]
    for n, p in counts:
        print(f"{n:6d} {p}")
    print(f"{sum(n for n, _ in counts):6d} total")
