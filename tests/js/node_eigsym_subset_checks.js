'use strict';
/* Node-side checks of eigen_sym / eigenvals_sym with opts.subset through the JS host and the N-API addon. Driven by
 * tests/test_node_eigsym_subset.py.
 *   node node_eigsym_subset_checks.js cpu                 (no GPU: the argument errors of opts.subset, the empty subset)
 *   node node_eigsym_subset_checks.js gpu <cases.json>    (GPU: host arrays and DeviceNDArrays give the bits of the Python result)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_sym', 'eigenvals_sym'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;
const eye = N => { const d = new Float64Array(N * N); for (let i = 0; i < N; i++) d[i * N + i] = 1; return new la.NDArray(Int32Array.of(N, N), d); };

function subsetErrors() {
  for (const fn of NAMES) {
    for (const bad of [[3, 2], [-1, 2], [0, 5], [0], [0, 1, 2], 3, [0.5, 2], 'ab'])
      assert.throws(() => la[fn](eye(4), {subset: bad}), err => /subset must be \[i0, i1\] with 0 <= i0 <= i1 <= N/.test(err.message), `${fn} ${JSON.stringify(bad)}`);
    assert.throws(() => la[fn](eye(4), {subset: [0, 1], algo: 'jacobi'}), /subset is not available with algo 'jacobi'/, fn);
  }
}

if (mode === 'cpu') {
  subsetErrors();
  // an NDArray has no axis of length 0 (the reference's constructor refuses it), so the JS layer refuses the empty subset
  for (const fn of NAMES) assert.throws(() => la[fn](eye(4), {subset: [2, 2]}), /the subset \[2, 2\] is empty/, fn);
  console.log('node eigsym subset cpu checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const shape = Int32Array.from(c.shape), N = shape[shape.length - 1], k = c.subset[1] - c.subset[0];
    const data = Float64Array.from(c.S), S = new la.NDArray(shape, data), keep = Float64Array.from(data), opts = {subset: c.subset};
    const lamWant = Float64Array.from(c.lam), vWant = Float64Array.from(c.V), lead = Array.from(shape.subarray(0, shape.length - 2));
    const [lam, V] = la.eigen_sym(S, opts);
    assert(lam instanceof la.NDArray && V instanceof la.NDArray, name + ' host in, host out');
    assert.deepStrictEqual(Array.from(lam.shape), lead.concat([k]), name); assert.deepStrictEqual(Array.from(V.shape), lead.concat([N, k]), name);
    assert(sameBits(lam.data, lamWant) && sameBits(V.data, vWant), name + ': other bits than the Python result');
    assert(sameBits(data, keep), name + ': S was written');
    assert(sameBits(la.eigenvals_sym(S, opts).data, lamWant), name + ': eigenvals_sym has other bits');
    const Sd = la.to_device(S), [ld, Vd] = la.eigen_sym(Sd, opts), l2 = la.eigenvals_sym(Sd, opts);
    assert(ld instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray && l2 instanceof la.DeviceNDArray, name + ' device in, device out');
    assert.deepStrictEqual(Array.from(Vd.shape), lead.concat([N, k]), name);
    assert(sameBits(la.to_host(ld).data, lamWant) && sameBits(la.to_host(Vd).data, vWant) && sameBits(la.to_host(l2).data, lamWant), name + ' device bits');
    assert(sameBits(la.to_host(Sd).data, keep), name + ': the device S was written');
    n++;
  }
  subsetErrors();
  const bad = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, NaN, 1));
  assert.throws(() => la.eigen_sym(bad, {subset: [0, 1]}), /NaN or Infinity in its lower triangle/);
  console.log('node eigsym subset gpu checks ok', n);
} else throw new Error('mode');
