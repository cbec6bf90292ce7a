"""Code lines of Python files: lines that carry a token other than a comment, with docstrings (a string that is a statement of its
own) left out.  Blank lines, comments and docstrings do not count; a statement over three lines counts three.
  python tools/code_lines.py memo_amd/*.py bin/memo          # per file and the total
"""
import ast
import sys
import tokenize

SKIP = {tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING, tokenize.ENDMARKER}


def code_lines(path):
    with open(path, "rb") as fh:
        source = fh.read()
    doc = set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant) and isinstance(node.value.value, str):
            doc.update(range(node.lineno, node.end_lineno + 1))
    with open(path, "rb") as fh:
        lines = {line for tok in tokenize.tokenize(fh.readline) if tok.type not in SKIP for line in range(tok.start[0], tok.end[0] + 1)}
    return len(lines - doc)


if __name__ == "__main__":
    total = 0
    for path in sys.argv[1:]:
        n = code_lines(path)
        total += n
        print(f"{n:6d} {path}")
    print(f"{total:6d} total")
